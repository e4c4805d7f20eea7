"""The yardstick of the lDDT tests: a float64 numpy restatement of the definition in include/str2str_hip.h, with square roots, written the
obvious way.

    P(a) = {(i, j) ordered : |i - j| >= min_seq_sep, d_a(i, j) < cutoff}
    hits = sum over P(a) of #{t in (0.5, 1, 2, 4) : |d_a(i, j) - d_b(i, j)| < t},   lDDT(a -> b) = hits / (4 |P(a)|), 1.0 for an empty P(a)

tests/test_ensemble_lddt_cpu.py holds it to the reference's own ``lddt`` (src/models/loss.py:384-437) through tests/golden/lddt.npz and to
cases worked by hand.  ``margin`` is the distance of a case from the nearest comparison that could flip: the device compares squared
distances with squared bounds, a few ulp of 15 A ~ 1e-14 A away from these, so a case is a parity input while its margin is >= MARGIN.
"""
import numpy as np

THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
MARGIN = 1e-10


def distances(x):
    """x [..., L, 3] -> d [..., L, L] float64."""
    x = np.asarray(x, dtype=np.float64)
    d = x[..., :, None, :] - x[..., None, :, :]
    return np.sqrt((d * d).sum(-1))


def separated(L, min_seq_sep=1):
    i = np.arange(L)
    return np.abs(i[:, None] - i[None, :]) >= min_seq_sep


def counts(a, b, cutoff=15.0, min_seq_sep=1):
    """One reference a [L, 3] and models b [R, L, 3] -> (hits [R, L] int64: per residue i over its included pairs, n [L] int64: included
    partners of residue i)."""
    da, db = distances(a), distances(b)
    with np.errstate(invalid="ignore"):
        inc = separated(len(da), min_seq_sep) & (da < cutoff)
        l1 = np.abs(da[None] - db)
        score = sum((l1 < t).astype(np.int64) for t in THRESHOLDS)
    return (score * inc[None]).sum(-1), inc.sum(-1).astype(np.int64)


def _ratio(hits, n):
    hits, n = np.broadcast_arrays(np.asarray(hits, dtype=np.float64), np.asarray(n, dtype=np.float64))
    out = np.ones(hits.shape)
    np.divide(hits, 4.0 * n, out=out, where=n > 0)
    return out


def per_residue(model, target, cutoff=15.0, min_seq_sep=1):
    """model [R, L, 3] against the reference target [L, 3] -> (per_res [R, L], total [R]) float64."""
    hits, n = counts(target, model, cutoff, min_seq_sep)
    return _ratio(hits, n[None]), _ratio(hits.sum(-1), n.sum())


def matrix(a, b, cutoff=15.0, min_seq_sep=1):
    """Every structure of a [Ra, L, 3] as the reference of every structure of b [Rb, L, 3] -> lDDT [Ra, Rb] float64."""
    return np.stack([per_residue(b, x, cutoff, min_seq_sep)[1] for x in a])


def symmetrised(x, cutoff=15.0, min_seq_sep=1):
    """min(lDDT(i -> j), lDDT(j -> i)) of an ensemble x [R, L, 3] -> [R, R]."""
    m = matrix(x, x, cutoff, min_seq_sep)
    return np.minimum(m, m.T)


def margin(a, b, cutoff=15.0, min_seq_sep=1):
    """The smallest of | |d_a - d_b| - t | over the included pairs of every (a[i], b[j]) and the four t, and of |d_a - cutoff| over the pairs
    with |i - j| >= min_seq_sep (inf where there is no such pair)."""
    da, db = distances(a), distances(b)
    sep = separated(da.shape[-1], min_seq_sep)
    worst = np.inf
    if sep.any():
        worst = float(np.abs(da[:, sep] - cutoff).min())
    for x in da:
        inc = sep & (x < cutoff)
        if inc.any():
            l1 = np.abs(x[inc][None] - db[:, inc])
            worst = min(worst, min(float(np.abs(l1 - t).min()) for t in THRESHOLDS))
    return worst
