"""The inputs of the time-lagged covariance and TICA tests (tests/test_ensemble_tica*.py) and their float64 yardstick values
(tests/ref_tica.py), built once and shared read-only.

Bounds (the project's reordered-sum rule with u = 2^-52; each side is within (terms - 1) u / 2 of the exact sum relative to the sum of the
terms' magnitudes, and 16 covers the roundings of one term: the widening, the subtraction of the mean, the sqrt(2n) scaling, the products):

    |mean - ref|        <= (2n + 16) u sum_t (|f_t| + |f_{t+lag}|) / 2n
    |C[r, c] - ref|     <= (2n + 16) u sum of the terms' CENTRED magnitudes   (what the offset cases are for: a one-pass
                                                                               E[xy] - E[x] E[y] fails them by 100^2)
    |proj[s, k] - ref|  <= (D + 16) u sum_c |z_sc| |v_kc|

Conditions on the end-to-end cases, asserted on the CPU (tests/test_ensemble_tica_cpu.py): no eigenvalue of the reference C00 within 1e-6
relative of the cut-off, every reference projection at least 1e-9 of the range away from a histogram edge, the fixture's unrounded js_tica
at least 1e-6 away from a rounding boundary of the fourth decimal."""
import functools

import numpy as np

import ref_tica as ref
from conftest import golden
from oracle import tica as OT

U52 = 2.0 ** -52
WAVE_SLOTS, MIN_GROUP_PAIRS = 1024, 512                      # S2S_TICA_WAVE_SLOTS, S2S_TICA_MIN_GROUP_PAIRS of include/str2str_hip.h


def groups(n, D):
    """The header's rule (S2S_TICA_GROUPS, S2S_TICA_GROUP_PAIRS), restated: -> (G, pairs per group)."""
    blocks = (D + 47) // 48
    n4 = (n + 3) // 4 * 4
    wanted = max(1, min(WAVE_SLOTS // (blocks * (blocks + 1) // 2), (n4 + MIN_GROUP_PAIRS - 1) // MIN_GROUP_PAIRS))
    group = (n4 // 4 + wanted - 1) // wanted * 4
    return (n4 + group - 1) // group, group


SPLIT_D, SPLIT_LAG = 45, 20
SPLIT_T = next(T for T in range(SPLIT_LAG + 1, 1 << 16) if groups(T - SPLIT_LAG, SPLIT_D)[0] > 1)   # the smallest T with G > 1 at D = 45
# (T, D, lag): a partial tile with n = 5 no multiple of 4; one partial block; one feature into a second block (mirrors, an off-diagonal
# block); 2.5 blocks; n = 1; three blocks with one live feature in the last and two k-steps; the smallest T at which the pairs of D = 45
# are split into groups (it stays the last case)
CASES = ((6, 3, 1), (37, 45, 3), (130, 49, 20), (257, 120, 7), (21, 45, 20), (10, 97, 2), (SPLIT_T, SPLIT_D, SPLIT_LAG))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def features(T, D, lag, offset=False):
    """f [T, D] float32: a slow random walk seen through D random read-outs plus independent noise, centred at the origin or with every
    feature ``offset`` by 100."""
    rng = np.random.default_rng(100000 * T + 100 * D + lag)
    slow = np.cumsum(rng.normal(size=(T, 3)), axis=0) * 0.3
    f = slow @ rng.normal(size=(3, D)) + rng.normal(size=(T, D))
    f -= f.mean(0)
    if offset:
        f += 100.0
    return _frozen(f.astype(np.float32))[0]


@functools.lru_cache(maxsize=None)
def reference(T, D, lag, offset=False):
    """Route B of ``features`` -> (mean, C00, C0t, A00, A0t)."""
    return _frozen(*ref.explicit(features(T, D, lag, offset), lag))


def mean_bound(f, lag):
    n = len(f) - lag
    return (2 * n + 16) * U52 * ref.mean_magnitude(f, lag)


def cov_bound(magnitudes, n):
    return (2 * n + 16) * U52 * magnitudes


def proj_bound(magnitudes, D):
    return (D + 16) * U52 * magnitudes


# ------------------------------------------------------------------------------------------------------------------- end to end
TAGS = ("a", "b")
N_PERTURBATIONS = 8


@functools.lru_cache(maxsize=None)
def fixture(tag):
    """tests/golden/tica.npz, tag a (D = 66, lag 20) or b (D = 45, lag 5) -> (coordinates {"target", "pred"}, their CA-distance features,
    lag, weights of pred, the rounded js_tica, the rounded weighted js_tica)."""
    g = golden("tica.npz")
    ca = {"target": g[f"{tag}_target"], "pred": g[f"{tag}_pred"]}
    feats = {k: ref.pairwise_distances(v) for k, v in ca.items()}
    return ca, feats, int(g[f"{tag}_lag"]), g[f"{tag}_weights"], float(g[f"{tag}_js_tica"]), float(g[f"{tag}_js_tica_w"])


@functools.lru_cache(maxsize=None)
def oracle_fit(tag):
    """oracle.tica.TICA(dim=2) on the fixture's reference features."""
    _, feats, lag, *_ = fixture(tag)
    return OT.TICA(dim=2, lagtime=lag).fit(feats["target"])


@functools.lru_cache(maxsize=None)
def sensitivity(tag):
    """How far the a-priori rounding of the covariances can move TICA's results, MEASURED ON THE REFERENCE: the route-A covariances of the
    fixture's reference features are perturbed by N_PERTURBATIONS seeded symmetric matrices whose entries are uniform within +- the
    a-priori bound of ``cov_bound``, the oracle's tail runs on each, and the largest change of every quantity is kept
    -> {"eigenvalues", "components", "tic_target", "tic_pred"}."""
    _, feats, lag, *_ = fixture(tag)
    f = feats["target"]
    n = len(f) - lag
    mean, c00, c0t = ref.route_a(f, lag)
    _, _, _, a00, a0t = ref.explicit(f, lag)
    base = ref.Tail(mean, c00, c0t)
    rng = np.random.default_rng(2024 + ord(tag))
    s = dict.fromkeys(("eigenvalues", "components", "tic_target", "tic_pred"), 0.0)
    for _ in range(N_PERTURBATIONS):
        moved = []
        for c, a in ((c00, a00), (c0t, a0t)):
            e = np.triu(rng.uniform(-1.0, 1.0, size=c.shape) * cov_bound(a, n))
            moved.append(c + e + np.triu(e, 1).T)
        t = ref.Tail(mean, *moved)
        assert t.rank == base.rank
        s["eigenvalues"] = max(s["eigenvalues"], float(np.abs(t.eigenvalues[:2] - base.eigenvalues[:2]).max()))
        s["components"] = max(s["components"], float(np.abs(t.coefficients - base.coefficients).max()))
        for k in ("target", "pred"):
            s[f"tic_{k}"] = max(s[f"tic_{k}"], float(np.abs(t.transform(feats[k]) - base.transform(feats[k])).max()))
    return s
