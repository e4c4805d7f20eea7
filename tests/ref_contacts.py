"""The yardstick of the contact tests: the definitions of include/str2str_hip.h (contact, contact map, contact statistics, native contact
list, hard and soft Q) in plain float64 numpy, one structure at a time.  tests/test_ensemble_contacts_cpu.py guards this file with facts
it did not produce (an ideal helix, a straight strand, mixtures of the two).

    v(i, j) = (dx dx + dy dy) + dz dz on the widened coordinates;   contact(i, j)  <=>  j - i >= min_seq_sep and v < cutoff^2
"""
import numpy as np

CUTOFF, MIN_SEQ_SEP = 8.0, 3                 # the defaults of the map and the statistics
NATIVE_CUTOFF, NATIVE_MIN_SEQ_SEP = 8.0, 4   # ... of the native list (|i - j| > 3, Best, Hummer and Eaton 2013)
BETA, LAM = 5.0, 1.2                         # ... of Q (their values for CA models)
MARGIN = 1e-9                                # the least relative margin a device case may have


def sq_dist(x):
    """x [L, 3] -> v [L, L] float64."""
    x = np.asarray(x, dtype=np.float64)
    d = x[:, None, :] - x[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def eligible(L, min_seq_sep):
    """[L, L] bool: j - i >= min_seq_sep."""
    i = np.arange(L)
    return i[None, :] - i[:, None] >= min_seq_sep


def contacts(x, cutoff=CUTOFF, min_seq_sep=MIN_SEQ_SEP):
    """x [L, 3] -> [L, L] bool, upper triangle only.  A comparison with NaN is false."""
    with np.errstate(invalid="ignore"):
        return (sq_dist(x) < cutoff * cutoff) & eligible(len(x), min_seq_sep)


def contact_counts(ens, cutoff=CUTOFF, min_seq_sep=MIN_SEQ_SEP):
    """ens [R, L, 3] -> counts [L, L] int32, symmetric, zero inside the band."""
    L = ens.shape[1]
    n = np.zeros((L, L), dtype=np.int32)
    for x in ens:
        n += contacts(x, cutoff, min_seq_sep)
    return n + n.T


def weighted_map(ens, weights, cutoff=CUTOFF, min_seq_sep=MIN_SEQ_SEP):
    """-> sum_r w_r [contact_r] [L, L] float64, summed in ascending structure order, symmetric."""
    L = ens.shape[1]
    acc = np.zeros((L, L), dtype=np.float64)
    for x, w in zip(ens, np.asarray(weights, dtype=np.float64)):
        acc = acc + np.where(contacts(x, cutoff, min_seq_sep), w, 0.0)
    return acc + acc.T


def contact_probability(ens, cutoff=CUTOFF, min_seq_sep=MIN_SEQ_SEP, weights=None):
    if weights is None:
        return contact_counts(ens, cutoff, min_seq_sep) / float(len(ens))
    return weighted_map(ens, weights, cutoff, min_seq_sep) / np.asarray(weights, dtype=np.float64).sum()


def contact_stats(ens, cutoff=CUTOFF, min_seq_sep=MIN_SEQ_SEP):
    """-> (n_contacts [R] int32, sep_sum [R] int64: the sum of j - i over the contacts)."""
    L = ens.shape[1]
    sep = np.arange(L)[None, :] - np.arange(L)[:, None]
    n, s = np.zeros(len(ens), dtype=np.int32), np.zeros(len(ens), dtype=np.int64)
    for r, x in enumerate(ens):
        c = contacts(x, cutoff, min_seq_sep)
        n[r], s[r] = c.sum(), sep[c].sum()
    return n, s


def contact_order(n_contacts, sep_sum, L):
    """The relative contact order sep_sum / (L n_contacts), 0.0 without contacts."""
    n = np.asarray(n_contacts, dtype=np.float64)
    return np.where(n > 0, np.asarray(sep_sum, dtype=np.float64) / (L * np.maximum(n, 1.0)), 0.0)


def native_list(native, cutoff=NATIVE_CUTOFF, min_seq_sep=NATIVE_MIN_SEQ_SEP):
    """native [L, 3] -> (pairs [n, 2] int32 in ascending (i, j) order, d0 [n] float64)."""
    c = contacts(native, cutoff, min_seq_sep)
    return np.ascontiguousarray(np.argwhere(c), dtype=np.int32).reshape(-1, 2), np.sqrt(sq_dist(native)[c])


def _entry_sq_dist(x, pairs):
    x = np.asarray(x, dtype=np.float64)
    d = x[pairs[:, 0]] - x[pairs[:, 1]]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def native_q(ens, pairs, d0, beta=BETA, lam=LAM):
    """-> (q_soft [R], q_hard [R] float64, hits [R] int32); an empty list gives 1.0."""
    R, n = len(ens), len(pairs)
    q_soft, q_hard, hits = np.ones(R), np.ones(R), np.zeros(R, dtype=np.int32)
    if n == 0:
        return q_soft, q_hard, hits
    b = lam * d0
    for r, x in enumerate(ens):
        v = _entry_sq_dist(x, pairs)
        with np.errstate(invalid="ignore", over="ignore"):
            hits[r] = (v < b * b).sum()
            q_soft[r] = np.sum(1.0 / (1.0 + np.exp(beta * (np.sqrt(v) - b)))) / n
        q_hard[r] = hits[r] / float(n)
    return q_soft, q_hard, hits


def margin(ens, cutoff=CUTOFF, min_seq_sep=MIN_SEQ_SEP, pairs=None, d0=None, lam=LAM):
    """The least relative distance of any comparison from flipping: |v - c^2| / c^2 over the eligible pairs of every structure, or, with a
    list, |v - (lam d0)^2| / (lam d0)^2 over its entries.  inf when there is nothing to compare."""
    out = np.inf
    if pairs is None:
        ok, c2 = eligible(ens.shape[1], min_seq_sep), cutoff * cutoff
        for x in ens:
            v = sq_dist(x)[ok]
            if v.size:
                out = min(out, float(np.abs(v - c2).min() / c2))
    elif len(pairs):
        b2 = (lam * d0) * (lam * d0)
        for x in ens:
            out = min(out, float((np.abs(_entry_sq_dist(x, pairs) - b2) / b2).min()))
    return out
