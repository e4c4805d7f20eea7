"""The float64 numpy restatement of include/str2str_kinetics.h and of the host tail of metrics.msm / metrics.js_msm: the yardstick of
tests/test_kinetics.py, held to facts it did not produce by tests/test_kinetics_cpu.py.  A helper, not a test module.

Every definition is written the plain way, with nothing shared with the package: the squared distance is summed over the dimensions in
ascending order, a term at a time (not np.sum, whose pairwise order is another one); ties go to the lowest index (np.argmin and
np.argmax return the first extremum)."""
import numpy as np

PSEUDO_C = 1e-6


def dist2(x, centres):
    """[T, k]: sum_i (x_ti - c_ji)^2, i ascending, every operation rounded on its own."""
    x, centres = np.asarray(x, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    acc = np.zeros((x.shape[0], centres.shape[0]))
    for i in range(x.shape[1]):
        diff = x[:, i, None] - centres[None, :, i]
        acc = acc + diff * diff
    return acc


def assign(x, centres):
    """-> (labels int32 [T], the minimal squared distance [T], the relative gap between the best and the second best, inf for k = 1)."""
    d2 = dist2(x, centres)
    labels = np.argmin(d2, axis=1)
    best = d2[np.arange(len(d2)), labels]
    if d2.shape[1] == 1:
        return labels.astype(np.int32), best, np.inf
    second = np.partition(d2, 1, axis=1)[:, 1]
    gap = np.min((second - best) / np.maximum(second, np.finfo(np.float64).tiny))
    return labels.astype(np.int32), best, float(gap)


def update(x, labels, centres):
    """-> (counts [k], the new centres [k, d]: the mean of the members in float64 (math.fsum per coordinate: the exact sum, rounded once),
    an empty cluster keeping its centre; sum_t |x_t| per cluster and coordinate [k, d], for the bound of the test)."""
    import math

    x, centres = np.asarray(x, dtype=np.float64), np.array(centres, dtype=np.float64)
    k = centres.shape[0]
    counts, mags = np.zeros(k, dtype=np.int64), np.zeros_like(centres)
    for j in range(k):
        members = x[np.asarray(labels) == j]
        counts[j] = len(members)
        if len(members):
            centres[j] = [math.fsum(members[:, i]) / len(members) for i in range(x.shape[1])]
            mags[j] = np.abs(members).sum(0)
    return counts, centres, mags


def farthest_points(x, k, first=0):
    """-> (indices [k], centres [k, d], the smallest relative gap between the largest and the second largest minimal distance)."""
    x = np.asarray(x, dtype=np.float64)
    indices, gap = [int(first)], np.inf
    mind = dist2(x, x[first][None])[:, 0]
    for _ in range(1, k):
        at = int(np.argmax(mind))
        if len(mind) > 1:
            top = np.partition(mind, -2)[-2:]
            if top[1] > 0:
                gap = min(gap, float((top[1] - top[0]) / top[1]))
        indices.append(at)
        mind = np.minimum(mind, dist2(x, x[at][None])[:, 0])
    return np.asarray(indices, dtype=np.int32), x[indices].copy(), gap


def lloyd(x, centres, max_iter=100):
    """Assign, then update, until an assignment changes no label or max_iter assignments have run.
    -> dict(centres: the ones the returned labels were assigned against, labels, counts, inertia, n_iter, converged, gap: the smallest
    assignment gap over all iterations, empty: whether any update met an empty cluster)."""
    centres = np.array(centres, dtype=np.float64)
    prev, converged, gap, empty = None, False, np.inf, False
    for n_iter in range(1, max_iter + 1):
        labels, best, g = assign(x, centres)
        gap = min(gap, g)
        if prev is not None and (labels != prev).sum() == 0:
            converged = True
            break
        if n_iter < max_iter:
            counts, centres, _ = update(x, labels, centres)
            empty = empty or bool((counts == 0).any())
            prev = labels
    return dict(centres=centres, labels=labels, counts=np.bincount(labels, minlength=len(centres)), inertia=float(best.sum()), n_iter=n_iter,
                converged=converged, gap=gap, empty=empty)


def kmeans(x, k, first=0, max_iter=100):
    return lloyd(x, farthest_points(x, k, first)[1], max_iter)


def transition_counts(labels, k, lag, lengths=None):
    """[k, k] int64: the pairs (t, t + lag) inside one trajectory with both labels in 0 .. k-1."""
    labels = np.asarray(labels)
    counts = np.zeros((k, k), dtype=np.int64)
    start = 0
    for n in ([len(labels)] if lengths is None else lengths):
        traj = labels[start:start + n]
        start += n
        for t in range(len(traj) - lag):
            a, b = traj[t], traj[t + lag]
            if 0 <= a < k and 0 <= b < k:
                counts[a, b] += 1
    return counts


def active_set(counts):
    """The largest strongly connected set of counts > 0 by plain reachability (Warshall), the set with the lowest state on a size tie."""
    n = len(counts)
    reach = (np.asarray(counts) > 0) | np.eye(n, dtype=bool)
    for m in range(n):
        reach = reach | (reach[:, m, None] & reach[None, m, :])
    both = reach & reach.T
    sets = {tuple(np.flatnonzero(both[i])) for i in range(n)}
    return np.asarray(min(sets, key=lambda s: (-len(s), s[0])))


def row_normalised(c):
    c = np.asarray(c, dtype=np.float64)
    return c / c.sum(1)[:, None]


def reversible_mle(c, tol=1e-12, max_iter=100000, dtype=np.float64):
    """x_ij <- (c_ij + c_ji) / (c_i / x_i + c_j / x_j) from x = C + C^T until the relative residual of that equation is <= tol wherever
    c_ij + c_ji > 0.  -> (T, pi, converged, the residual reached)."""
    c = np.asarray(c, dtype=dtype)
    s, ci = c + c.T, c.sum(1)
    x, pair = s.copy(), s > 0
    converged, residual = False, np.inf
    for _ in range(max_iter):
        q = ci / x.sum(1)
        denom = q[:, None] + q[None, :]
        residual = (np.abs(x * denom - s)[pair] / s[pair]).max()
        if residual <= tol:
            converged = True
            break
        x = np.where(pair, s / np.where(pair, denom, 1), 0)
    xi = x.sum(1)
    return x / xi[:, None], xi / xi.sum(), converged, residual


def msm(counts, lagtime, reversible=True, tol=1e-12, max_iter=100000):
    """The host tail on a count matrix -> dict(active, transition_matrix, stationary, eigenvalues, timescales, converged)."""
    act = active_set(counts)
    c = np.asarray(counts)[np.ix_(act, act)].astype(np.float64)
    if len(act) == 1 and c[0, 0] == 0:
        t, pi, converged = np.ones((1, 1)), np.ones(1), True
    elif reversible:
        t, pi, converged, _ = reversible_mle(c, tol, max_iter)
    else:
        t, converged = row_normalised(c), True
        w, v = np.linalg.eig(t.T)
        pi = np.abs(np.real(v[:, np.argmin(np.abs(w - 1.0))]))
        pi = pi / pi.sum()
    root = np.sqrt(pi)
    sym = root[:, None] * t / root[None, :]
    lam = np.linalg.eigvalsh(0.5 * (sym + sym.T))
    lam = lam[np.argsort(-np.abs(lam), kind="stable")]
    mag = np.abs(lam[1:])
    with np.errstate(divide="ignore"):
        timescales = np.where(mag >= 1.0, np.inf, np.abs(-float(lagtime) / np.log(np.where(mag < 1.0, mag, 0.5))))
    return dict(active=act, transition_matrix=t, stationary=pi, eigenvalues=lam, timescales=timescales, converged=converged)


def js(p, q):
    """The Jensen-Shannon distance (natural logarithm) of two histograms."""
    p, q = p / p.sum(), q / q.sum()
    m = 0.5 * (p + q)
    kl = lambda a: float(np.sum(np.where(a > 0, a * np.log(np.where(a > 0, a, 1.0) / m), 0.0)))   # noqa: E731
    return float(np.sqrt(0.5 * (kl(p) + kl(q))))


def js_of_states(labels, k, ref_key="target", weights=None):
    """js_msm's histogram tail: {key: labels} -> {key: the rounded JS distance of the state histogram + PSEUDO_C from the reference's}."""
    hist = {key: np.bincount(lab, weights=(weights or {}).get(key), minlength=k) + PSEUDO_C for key, lab in labels.items()}
    return {key: 0.0 if key == ref_key else np.around(js(h, hist[ref_key]), decimals=4) for key, h in hist.items()}
