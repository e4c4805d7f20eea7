"""The yardstick of the clustering tests: the GROMOS algorithm (Daura et al. 1999; ``gmx cluster -method gromos``) restated in numpy on a
boolean neighbour matrix, one cluster per pass with no shortcut, and the bit packing of the device's adjacency layout."""
import numpy as np


def gromos(adj):
    """adj [n, n] bool, symmetric; the diagonal counts as set -> (labels [n], centres [K], sizes [K]) int32.  The live structure with the
    most live neighbours (np.argmax: the lowest index among equals) is the next centre; it and its live neighbours leave."""
    adj = np.asarray(adj, dtype=bool) | np.eye(len(adj), dtype=bool)
    live = np.ones(len(adj), dtype=bool)
    labels, centres, sizes = np.full(len(adj), -1, dtype=np.int32), [], []
    while live.any():
        count = np.where(live, (adj & live[None, :]).sum(1), -1)
        c = int(np.argmax(count))
        members = adj[c] & live
        labels[members] = len(centres)
        centres.append(c)
        sizes.append(int(members.sum()))
        live &= ~members
    return labels, np.asarray(centres, dtype=np.int32), np.asarray(sizes, dtype=np.int32)


def pack_bits(adj):
    """bool [n, n] -> uint64 [n, ceil(n / 64)]: bit j % 64 (little-endian) of word j // 64 of row i is adj[i, j]; padding bits are zero."""
    adj = np.asarray(adj, dtype=bool)
    n, W = adj.shape[1], -(-adj.shape[1] // 64)
    padded = np.zeros((adj.shape[0], W * 64), dtype=bool)
    padded[:, :n] = adj
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(adj.shape[0], W)


def integer_matrix(n, hi, seed):
    """The integer-valued test matrices: d = rng.integers(0, hi + 1, (n, n)) symmetrised from its upper triangle, zero diagonal, float64."""
    d = np.triu(np.random.default_rng(seed).integers(0, hi + 1, (n, n)), 1)
    return (d + d.T).astype(np.float64)


def random_walk(rng, L, step=3.8):
    s = rng.normal(size=(L, 3))
    s *= step / np.linalg.norm(s, axis=1, keepdims=True)
    return np.cumsum(s, axis=0)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def planted_ensemble(seed=7, L=24, copies=(40, 25, 12, 3), sigma=0.3):
    """Random-walk chains of L residues with 3.8 A steps, ``copies`` noisy copies (Gaussian, sigma A) of each, every copy under a random
    rotation and translation, in shuffled order -> (coords [R, L, 3] float32, group [R]: the chain each copy came from)."""
    rng = np.random.default_rng(seed)
    out, group = [], []
    for g, m in enumerate(copies):
        base = random_walk(rng, L)
        for _ in range(m):
            out.append((base + rng.normal(size=base.shape) * sigma) @ random_rotation(rng).T + rng.uniform(-50.0, 50.0, size=3))
            group.append(g)
    order = rng.permutation(len(out))
    return np.asarray(out, dtype=np.float32)[order], np.asarray(group)[order]


def kabsch_rmsd_matrix(x):
    """float64 SVD Kabsch (proper rotations) of every pair of x [R, L, 3] -> rmsd [R, R]."""
    d = np.asarray(x, dtype=np.float64)
    d = d - d.mean(1, keepdims=True)
    g = (d * d).sum((1, 2))
    u, s, vt = np.linalg.svd(np.einsum("ail,bim->ablm", d, d))
    lam = s[..., 0] + s[..., 1] + np.sign(np.linalg.det(u @ vt)) * s[..., 2]
    return np.sqrt(np.maximum((g[:, None] + g[None, :] - 2.0 * lam) / d.shape[1], 0.0))
