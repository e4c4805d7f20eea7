"""The deterministic inputs of the backbone-violation tests, shared by the CPU test (which asserts their margins), the device test and the
fixture script: full backbones N, CA, C, O, CB built atom by atom from ideal bond lengths and angles and chosen torsions."""
import functools

import numpy as np

from ref_violations import GLY, PRO, exists_from_aatype

# (L, R) of the device parity cases: nothing to compare; one connection; the smallest chain with a break; 65 atoms, one past a wave; an odd
# length; residues one past a wave; 1 025 atoms, one past a sweep of 1 024 threads; the long-chain launch (above 256 residues)
SHAPES = ((1, 3), (2, 1), (3, 5), (13, 17), (31, 9), (65, 17), (205, 4), (300, 3))

EXTENDED, COMPACT, NOISY = 1, 2, 3   # kinds of ensemble members, see ``ensemble``
_DEG = np.pi / 180.0


def _place(a, b, c, length, angle, torsion):
    """The atom bonded to c at ``length``, with the angle (b, c, new) and the torsion (a, b, c, new) in degrees."""
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    t, w = angle * _DEG, torsion * _DEG
    return c + length * (-np.cos(t) * bc + np.sin(t) * np.cos(w) * m + np.sin(t) * np.sin(w) * n)


def build_backbone(phi, psi, omega=None):
    """[L] torsions in degrees -> float64 [L, 5, 3] (N, CA, C, O, CB) with the ideal geometry the violation terms hold a chain to:
    C-N 1.329 A, CA-C-N 116.568 and C-N-CA 121.352 degrees."""
    L = len(phi)
    omega = np.full(L, 180.0) if omega is None else omega
    x = np.zeros((L, 5, 3))
    x[0, 0], x[0, 1] = (0.0, 0.0, 0.0), (1.458, 0.0, 0.0)
    x[0, 2] = x[0, 1] + 1.525 * np.array([-np.cos(111.0 * _DEG), np.sin(111.0 * _DEG), 0.0])
    for k in range(L):
        n, ca, c = x[k, 0], x[k, 1], x[k, 2]
        x[k, 3] = _place(n, ca, c, 1.231, 120.8, psi[k] + 180.0)
        b, cc = ca - n, c - ca
        x[k, 4] = -0.58273431 * np.cross(b, cc) + 0.56802827 * b - 0.54067466 * cc + ca
        if k + 1 < L:
            x[k + 1, 0] = _place(n, ca, c, 1.329, 116.568, psi[k])
            x[k + 1, 1] = _place(ca, c, x[k + 1, 0], 1.458, 121.352, omega[k])
            x[k + 1, 2] = _place(c, x[k + 1, 0], x[k + 1, 1], 1.525, 111.0, phi[k + 1])
    return x


def sequence(rng, L, with_break=True):
    """-> (aatype [L] with a GLY and a PRO where the chain has room, residue_index [L] with one gap of three numbers in the middle)."""
    aatype = rng.integers(0, 20, size=L)
    aatype[aatype == GLY] = 0
    aatype[aatype == PRO] = 0
    if L == 1:
        aatype[0] = GLY
    else:
        aatype[0 if L < 4 else L // 3] = GLY
        aatype[L - 1 if L < 4 else (2 * L) // 3] = PRO
    ri = np.arange(L) + 5
    if with_break and L >= 3:
        ri[(L + 1) // 2:] += 3
    return aatype.astype(np.int64), ri.astype(np.int64)


def _gly_cb_decoy(x, aatype):
    """The CB slot of a GLY does not exist; what its coordinates hold must not matter.  Put it on the next residue's N (the previous one's C
    at the end of the chain): counted, it would clash."""
    L = len(aatype)
    for k in np.nonzero(aatype == GLY)[0]:
        if L > 1:
            x[..., k, 4, :] = x[..., k + 1, 0, :] if k + 1 < L else x[..., k - 1, 2, :]
    return x


@functools.lru_cache(maxsize=None)
def ensemble(L, R):
    """-> (atoms [R, L, 5, 3] float32, atom_exists [L, 5] bool, aatype [L], residue_index [L]), read-only.  Member r is of kind
    ``kind_of(r, R)``: 0 an extended random coil (ideal geometry, chance overlaps of residues far apart in sequence), EXTENDED its residues
    pulled 20 A apart from each other (every connection torn, NO residue pair passes the prefilter), COMPACT the coil shrunk to a
    two-hundredth (EVERY pair passes it and every counted atom pair clashes), 3 the coil with 0.08 A of noise on every atom (part of the
    connections violated), 4 a noisy helix."""
    rng = np.random.default_rng(9000 + 7 * L + R)
    aatype, ri = sequence(rng, L)
    out = np.zeros((R, L, 5, 3))
    for r in range(R):
        kind = kind_of(r, R)
        if kind == 4:
            x = build_backbone(-60.0 + rng.normal(size=L) * 8.0, -45.0 + rng.normal(size=L) * 8.0) + rng.normal(size=(L, 5, 3)) * 0.05
        else:
            x = build_backbone(rng.uniform(-180.0, 180.0, size=L), rng.uniform(-180.0, 180.0, size=L))
        if kind == NOISY:
            x += rng.normal(size=x.shape) * 0.08
        elif kind == EXTENDED:
            x += (np.arange(L) * 20.0)[:, None, None] * np.array([1.0, 0.0, 0.0])
        elif kind == COMPACT:
            x *= 0.005
        out[r] = x
    out = _gly_cb_decoy(out, aatype).astype(np.float32)
    exists = exists_from_aatype(aatype)
    for a in (out, exists, aatype, ri):
        a.setflags(write=False)
    return out, exists, aatype, ri


def kind_of(r, R):
    """A single structure is the noisy coil."""
    return r % 5 if R > 1 else NOISY


@functools.lru_cache(maxsize=None)
def fixture_cases():
    """The cases of tests/golden/violations.npz -> {tag: (atoms [L, 5, 3] float32, atom_exists, aatype, residue_index)}: chains of 12 and
    40 residues from ideal frames with perturbed helix / strand torsions, a GLY, a PRO and one chain break in each;
    ``stretched`` one C-N bond pulled 0.4 A apart, ``o_n`` the O of residue 3 put 1.2 A from the N of residue 30, ``hairpin`` the second
    half of the chain laid back over the first so that several atoms overlap."""
    rng = np.random.default_rng(77)
    cases = {}
    for tag, L in (("ideal12", 12), ("ideal40", 40), ("stretched", 12), ("o_n", 40), ("hairpin", 40)):
        aatype, ri = sequence(rng, L)
        strand = rng.random(L) < 0.3
        phi = np.where(strand, -120.0, -60.0) + rng.normal(size=L) * 10.0
        psi = np.where(strand, 130.0, -45.0) + rng.normal(size=L) * 10.0
        x = build_backbone(phi, psi)
        if tag == "stretched":
            step = x[5, 0] - x[4, 2]
            x[5:] += 0.4 * step / np.linalg.norm(step)
        elif tag == "o_n":
            v = rng.normal(size=3)
            x[3, 3] = x[30, 0] + 1.2 * v / np.linalg.norm(v)
        elif tag == "hairpin":
            x = build_backbone(np.full(L, -120.0) + rng.normal(size=L) * 3.0, np.full(L, 130.0) + rng.normal(size=L) * 3.0)
            x[20:] = x[19::-1] + np.array([0.9, 0.7, 0.5]) + rng.normal(size=(20, 5, 3)) * 0.2   # residue 20 + k lies over residue 19 - k
        x = _gly_cb_decoy(x, aatype).astype(np.float32)
        cases[tag] = (x, exists_from_aatype(aatype), aatype, ri)
        for a in cases[tag]:
            a.setflags(write=False)
    return cases
