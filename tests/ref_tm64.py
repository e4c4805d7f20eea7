"""The yardstick of the TM-score tests: a float64 numpy restatement of the definition in include/str2str_hip.h, and the input recipe.

    TM(a, b) = max over the evaluated superpositions (R proper, t) of (1/L) sum_i f_i,   f_i = 1 / (1 + |R a_i + t - b_i|^2 / d0^2)

Search: for every seed window (s, n), weights 1 on residues s .. s+n-1 and 0 elsewhere; 33 times: weighted Kabsch of a onto b, evaluate
f and the score, w <- f^2; the maximum over all seeds and evaluations.  The Kabsch here is ``np.linalg.svd`` of the weighted
cross-covariance with the determinant fix -- on purpose a different route from the kernel's eigen-quaternion by Jacobi.  Everything is
vectorised over pairs and seeds.  tests/test_ensemble_tm_cpu.py guards this file (monotone steps, planted motifs, seed counts).
"""
import numpy as np

ITERS = 33
SIGMAS = (1e-3, 0.05, 0.5, 2.0, 8.0)
N_KINDS = 8


# ------------------------------------------------------------------------------------------------------------------ input recipe
def random_walk(rng, L):
    step = rng.normal(size=(L, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
    return np.cumsum(step, axis=0)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def rigid_move(rng, x):
    """x under a random proper rotation and a translation of up to 50 A per axis."""
    return x @ random_rotation(rng).T + rng.uniform(-50.0, 50.0, size=3)


def make_ensemble(rng, n, L, base, first_kind=0):
    """n structures [n, L, 3] float32 around ``base``: exact copies, copies with Gaussian noise of the SIGMAS, unrelated chains and mirror
    images, in turn; each under its own rigid move."""
    out = []
    for s in range(n):
        kind = (s + first_kind) % N_KINDS
        if kind == 0:
            x = base.copy()
        elif kind <= 5:
            x = base + rng.normal(size=base.shape) * SIGMAS[kind - 1]
        elif kind == 6:
            x = random_walk(rng, L)
        else:
            x = base * np.array([-1.0, 1.0, 1.0])
        out.append(rigid_move(rng, x))
    return np.asarray(out, dtype=np.float32)


def planted_pair(rng, L):
    """(a, b [L, 3] float32, planted fraction): b repeats the first L // 2 residues of a (rigidly moved, as is the rest) and continues with
    an unrelated chain."""
    a = random_walk(rng, L)
    keep = L // 2
    tail = random_walk(rng, L - keep) + a[keep - 1]
    b = rigid_move(rng, np.concatenate([a[:keep], tail @ random_rotation(rng).T]))
    return np.asarray(rigid_move(rng, a), dtype=np.float32), np.asarray(b, dtype=np.float32), keep / L


# -------------------------------------------------------------------------------------------------------------------- definition
def tm_d0(L):
    return max(0.5, 1.24 * np.cbrt(L - 15.0) - 1.8) if L > 15 else 0.5


def tm_seeds(L):
    """The seed windows (start, length) in the order of the definition, duplicates (small L) included."""
    out = [(0, L)]
    for div in (2, 4):
        n = max(L // div, 4)
        if n >= L:
            continue
        stride = max(n // 2, 1)
        starts = list(range(0, L - n + 1, stride))
        out += [(s, n) for s in starts]
        if starts[-1] + n < L:
            out.append((L - n, n))
    return out


def kabsch(a, b, w):
    """Weighted Kabsch of a onto b ([..., L, 3] float64, w [..., L]) -> proper rotation R [..., 3, 3] and t [..., 3]: R a + t ~ b."""
    ws = w.sum(-1)[..., None]
    wa = w[..., None] * a
    ca, cb = wa.sum(-2) / ws, (w[..., None] * b).sum(-2) / ws
    h = np.swapaxes(wa - w[..., None] * ca[..., None, :], -1, -2) @ (b - cb[..., None, :])      # sum w (a - ca)(b - cb)^T
    rot = _proper_rotation(h)
    return rot, cb - np.einsum("...ij,...j->...i", rot, ca)


def score_under(a, b, rot, t, d0):
    """-> (f [..., L], score [...]) of the superposition (rot, t)."""
    d = a @ np.swapaxes(rot, -1, -2) + t[..., None, :] - b
    f = 1.0 / (1.0 + (d * d).sum(-1) / (d0 * d0))
    return f, f.mean(-1)


def _proper_rotation(h):
    """The proper rotation maximising tr(R H), H [..., 3, 3] = sum w a b^T: R = V diag(1, 1, det) U^T."""
    u, _, vt = np.linalg.svd(h)
    u[..., :, 2] *= np.sign(np.linalg.det(u @ vt))[..., None]
    return np.swapaxes(u @ vt, -1, -2)


def tm_search(a, b, d0=None, iters=ITERS, direct=False):
    """a, b [P, L, 3] (paired) -> dict: tm [P]; rot [P, 3, 3], trans [P, 3] of the evaluation that scored it (the first to reach the
    maximum, seeds in order); trace [seeds, iters, P], the score of every evaluation.
    Each structure is first moved to its own centroid (the search is translation invariant), so that the weighted Kabsch can work from the
    16 moments W, sum w a, sum w b, sum w a b^T -- one product of the weights with a fixed [L, 16] table per pair -- without cancellation;
    ``direct=True`` calls ``kabsch`` on the raw coordinates instead (slow; the CPU tests hold the two together)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    P, L = a.shape[:2]
    d0 = tm_d0(L) if d0 is None else float(d0)
    seeds = list(dict.fromkeys(tm_seeds(L)))
    w = np.zeros((P, len(seeds), L))
    for k, (s, n) in enumerate(seeds):
        w[:, k, s:s + n] = 1.0
    a0, b0 = (a.mean(1, keepdims=True), b.mean(1, keepdims=True)) if not direct else (np.zeros((P, 1, 3)), np.zeros((P, 1, 3)))
    ac, bc = a - a0, b - b0
    table = np.concatenate([np.ones((P, L, 1)), ac, bc, (ac[..., :, None] * bc[..., None, :]).reshape(P, L, 9)], -1)
    trace, rots, ts = [], [], []
    for _ in range(iters):
        if direct:
            rot, t = kabsch(np.broadcast_to(ac[:, None], w.shape + (3,)), np.broadcast_to(bc[:, None], w.shape + (3,)), w)
        else:
            m = w @ table                                        # [P, seeds, 16]
            ca, cb = m[..., 1:4] / m[..., :1], m[..., 4:7] / m[..., :1]
            rot = _proper_rotation(m[..., 7:].reshape(m.shape[:2] + (3, 3)) - m[..., 1:4, None] * cb[..., None, :])
            t = cb - np.einsum("...ij,...j->...i", rot, ca)
        f, score = score_under(ac[:, None], bc[:, None], rot, t, d0)
        trace.append(score); rots.append(rot); ts.append(t)
        w = f * f
    trace = np.stack(trace, 0).transpose(2, 0, 1)                # [seeds, iters, P]
    flat = trace.reshape(-1, P)
    top = flat.argmax(0)                                         # (the first maximum: seeds in order, then iterations)
    k, it = np.divmod(top, iters)
    rot, t = np.stack(rots)[it, np.arange(P), k], np.stack(ts)[it, np.arange(P), k]
    return {"tm": flat[top, np.arange(P)], "rot": rot, "trans": t + b0[:, 0] - np.einsum("pij,pj->pi", rot, a0[:, 0]), "trace": trace}


def tm_matrix(a, b, d0=None, iters=ITERS):
    """Every structure of a [Ra, L, 3] against every structure of b [Rb, L, 3] -> TM [Ra, Rb] float64."""
    na, nb = len(a), len(b)
    i, j = np.divmod(np.arange(na * nb), nb)
    return tm_search(np.asarray(a)[i], np.asarray(b)[j], d0, iters)["tm"].reshape(na, nb)


def kabsch_tm(a, b, d0=None):
    """The score of the plain unweighted Kabsch (minimum-RMSD) superposition of every pair -> [Ra, Rb]: a floor for the search."""
    na, nb = len(a), len(b)
    i, j = np.divmod(np.arange(na * nb), nb)
    x, y = np.asarray(a, dtype=np.float64)[i], np.asarray(b, dtype=np.float64)[j]
    rot, t = kabsch(x, y, np.ones(x.shape[:2]))
    return score_under(x, y, rot, t, tm_d0(x.shape[1]) if d0 is None else d0)[1].reshape(na, nb)


def perturbed(x, rng, rel=1e-15):
    """The widened coordinates moved by ``rel`` relative: the second evaluation that exposes an ill-conditioned pair."""
    x = np.asarray(x, dtype=np.float64)
    return x * (1.0 + rel * rng.standard_normal(x.shape))
