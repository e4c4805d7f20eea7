"""tests/ref_kinetics.py held to facts it did not produce, and everything of the kinetics family that needs no device: the k x k host tail
of metrics.msm against the restatement, the header against the binding, the argument checks, the eval switch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import kinetics_cases as KC
import ref_kinetics as RK
from conftest import ROOT, record_margin

EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ the restatement against planted facts
def _planted(seed=5, per=40, d=3, k=4):
    """k blobs of unit width whose centres are 50 widths apart along a line -> (x shuffled, the planted blob of every row)."""
    rng = np.random.default_rng(seed)
    centres = np.zeros((k, d))
    centres[:, 0] = 50.0 * np.arange(k)
    blob = rng.permutation(np.repeat(np.arange(k), per))
    return centres[blob] + rng.standard_normal((len(blob), d)), blob


def _same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def test_planted_blobs_are_recovered_exactly():
    x, blob = _planted()
    res = RK.kmeans(x, 4)
    assert res["converged"] and _same_partition(res["labels"], blob) and res["counts"].tolist() == [40] * 4
    for j in range(4):                                         # every centre is the mean of its blob, to rounding
        assert np.abs(res["centres"][j] - x[res["labels"] == j].mean(0)).max() <= 64 * EPS * 200.0
    assert res["inertia"] == pytest.approx(((x - res["centres"][res["labels"]]) ** 2).sum(), rel=1e-12)
    seeds = RK.farthest_points(x, 4)[0]
    assert seeds[0] == 0 and sorted(blob[seeds].tolist()) == [0, 1, 2, 3]      # one seed per blob: 50 widths apart beats any spread inside


def test_ties_go_to_the_lowest_index():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [4.0, 0.0]])
    centres = np.array([[4.0, 0.0], [0.0, 0.0], [0.0, 0.0], [4.0, 0.0]])          # centres 1, 2 and 0, 3 are duplicates
    labels, best, _ = RK.assign(x, centres)
    assert labels.tolist() == [1, 1, 0] and best.tolist() == [0.0, 1.0, 0.0]
    labels, _, _ = RK.assign(np.array([[2.0, 0.0]]), centres)                     # equidistant from all four
    assert labels.tolist() == [0]
    # farthest point: rows 1 and 2 are equally far from row 0; then every row left is at distance 0 from a chosen one
    idx, ctr, _ = RK.farthest_points(np.array([[0.0], [3.0], [-3.0], [0.0]]), 4)
    assert idx.tolist() == [0, 1, 2, 0] and ctr[:, 0].tolist() == [0.0, 3.0, -3.0, 0.0]


def test_an_empty_cluster_keeps_its_centre():
    x = np.array([[0.0, 1.0], [2.0, 3.0], [10.0, 10.0]])
    centres = np.array([[0.1, 0.2], [123.456, -7.0 / 3.0], [9.0, 9.0]])
    counts, new, mags = RK.update(x, np.array([0, 0, 2]), centres)
    assert counts.tolist() == [2, 0, 1] and new[1].tobytes() == centres[1].tobytes()
    assert new[0].tolist() == [1.0, 2.0] and new[2].tolist() == [10.0, 10.0] and mags[0].tolist() == [2.0, 4.0]
    assert centres[0].tolist() == [0.1, 0.2]                                      # (the input is left alone)


def test_transition_counts_of_a_hand_written_string():
    #          trajectory A (7 frames)      trajectory B (3)   C (1)
    labels = [0, 0, 1, -1, 1, 0, 2,         2, 2, 0,           1]
    lengths = [7, 3, 1]
    c1 = RK.transition_counts(labels, 3, 1, lengths)
    # A: 0>0, 0>1, (1>-1), (-1>1), 1>0, 0>2; B: 2>2, 2>0; C: nothing; the pair (2, 2) across A|B and (0, 1) across B|C do not count
    assert c1.tolist() == [[1, 1, 1], [1, 0, 0], [1, 0, 1]]
    c2 = RK.transition_counts(labels, 3, 2, lengths)
    # A: 0>1, (0>-1), 1>1, (-1>0), 1>2; B: 2>0
    assert c2.tolist() == [[0, 1, 0], [0, 1, 1], [1, 0, 0]]
    c3 = RK.transition_counts(labels, 3, 3, lengths)            # lag = the length of B: only A counts: (0>-1), 0>1, 1>0, (-1>2)
    assert c3.tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0]]
    assert RK.transition_counts(labels, 3, 7, lengths).sum() == 0 and RK.transition_counts(labels, 3, 1).sum() == 8
    assert RK.transition_counts(labels, 2, 1, lengths).tolist() == [[1, 1], [1, 0]]      # a label >= k is unassigned too


def test_active_set_is_the_largest_strongly_connected_set():
    c = np.zeros((6, 6), dtype=np.int64)
    c[0, 1] = c[1, 0] = 1                 # {0, 1}
    c[2, 3] = c[3, 4] = c[4, 2] = 1       # {2, 3, 4}: a cycle
    c[1, 2] = 5                           # one way only: does not join them
    assert RK.active_set(c).tolist() == [2, 3, 4]
    c[4, 2] = 0                           # now {2}, {3}, {4} are singletons: {0, 1} is the largest
    assert RK.active_set(c).tolist() == [0, 1]
    c[0, 1] = 0
    c[3, 2] = 1                           # {2, 3} against singletons
    assert RK.active_set(c).tolist() == [2, 3]
    c[5, 4] = c[4, 5] = 1                 # {2, 3} and {4, 5}: a tie, the set with the lowest state
    assert RK.active_set(c).tolist() == [2, 3]
    assert RK.active_set(np.zeros((3, 3))).tolist() == [0]


def test_two_state_reversible_estimate_is_the_row_normalised_one():
    """Every two-state chain is reversible, so the maximum-likelihood estimates with and without the constraint coincide.  The tolerance
    is 4 x the distance between the restatement at tol = 1e-12 in float64 and at tol = 1e-15 in np.longdouble (measured, recorded)."""
    from str2str_amd.metrics import metrics

    worst = 0.0
    for c in ([[90, 10], [4, 46]], [[5, 1], [3, 500]], [[1000, 3], [7, 20]]):
        c = np.array(c)
        t, pi, ok, _ = RK.reversible_mle(c)
        tl, pil, okl, _ = RK.reversible_mle(c, tol=1e-15, dtype=np.longdouble)
        assert ok and okl
        measured = float(max(np.abs(t - tl).max(), np.abs(pi - pil).max()))
        p = RK.row_normalised(c)                                                   # its stationary distribution is (p_10, p_01) / (p_01 + p_10)
        got = float(max(np.abs(t - p).max(), np.abs(pi - np.array([p[1, 0], p[0, 1]]) / (p[0, 1] + p[1, 0])).max()))
        print(f"two-state {c.tolist()}: measured {measured:.3e}, against the row-normalised counts {got:.3e}")
        assert measured > 0.0 and got <= 4.0 * measured
        worst = max(worst, got / measured)
        tm, pim, okm = metrics._reversible_mle(c, 1e-12, 100000)                   # the package's estimator: the same arithmetic
        assert okm and np.abs(tm - t).max() <= 4.0 * measured and np.abs(pim - pi).max() <= 4.0 * measured
    record_margin("MSM two-state: reversible MLE vs row-normalised counts (units of the longdouble distance)", worst, 4.0)


def _short_trajectories(n_traj=12, length=30, seed=2):
    rng = np.random.default_rng(seed)
    p = np.array([[0.8, 0.15, 0.05], [0.3, 0.6, 0.1], [0.05, 0.25, 0.7]])          # not reversible
    trajs = []
    for _ in range(n_traj):
        s = [int(rng.integers(0, 3))]
        for _ in range(length - 1):
            s.append(int(rng.choice(3, p=p[s[-1]])))
        trajs.append(s)
    return np.concatenate(trajs).astype(np.int32), [length] * n_traj


def test_reversible_fixed_point_on_short_trajectories():
    """Several short trajectories: the counts are far from symmetric, so x = C + C^T is far from the fixed point (a single long trajectory
    is almost one already and would test nothing)."""
    from str2str_amd.metrics import metrics

    labels, lengths = _short_trajectories()
    c = RK.transition_counts(labels, 3, 1, lengths)
    assert np.abs(c - c.T).max() >= 5
    first = RK.reversible_mle(c, max_iter=1)
    assert not first[2] and first[3] > 1e-3                                       # the start is no fixed point
    t, pi, ok, residual = RK.reversible_mle(c)
    assert ok and residual <= 1e-12
    flux = pi[:, None] * t
    assert np.abs(flux - flux.T).max() <= 4 * EPS * flux.max()                    # detailed balance, to rounding
    assert np.abs(t.sum(1) - 1.0).max() <= 5 * EPS and abs(pi.sum() - 1.0) <= 5 * EPS and (t >= 0).all()
    assert np.abs(pi @ t - pi).max() <= 8 * EPS                                   # pi is stationary
    assert np.abs(t - RK.row_normalised(c)).max() > 1e-3                          # and the constraint did something
    tm, pim, okm = metrics._reversible_mle(c, 1e-12, 100000)
    assert okm and np.array_equal(tm, t) and np.array_equal(pim, pi)


@pytest.mark.parametrize("reversible", (True, False))
def test_host_tail_of_msm_is_the_restatement(reversible):
    from str2str_amd.metrics import metrics

    labels, lengths = _short_trajectories()
    counts = np.zeros((5, 5), dtype=np.int64)
    counts[1:4, 1:4] = RK.transition_counts(labels, 3, 2, lengths)                 # states 0 and 4 are never visited
    got, want = metrics._msm_tail(counts, 2, reversible, 1e-12, 100000), RK.msm(counts, 2, reversible)
    assert got.active.tolist() == want["active"].tolist() == [1, 2, 3] and got.converged and got.lagtime == 2
    for name in ("transition_matrix", "stationary", "eigenvalues", "timescales"):
        assert np.allclose(getattr(got, name), want[name], rtol=1e-12, atol=0), name
    assert got.eigenvalues[0] == pytest.approx(1.0, abs=1e-12) and got.timescales.shape == (2,) and (got.timescales > 0).all()
    assert np.all(np.abs(got.eigenvalues[:-1]) >= np.abs(got.eigenvalues[1:]))
    assert metrics._active_set(counts).tolist() == [1, 2, 3]
    lone = metrics._msm_tail(np.zeros((3, 3), dtype=np.int64), 1, reversible, 1e-12, 10)
    assert lone.active.tolist() == [0] and lone.transition_matrix.tolist() == [[1.0]] and lone.timescales.shape == (0,)


def test_state_histograms_and_their_js_distance():
    from str2str_amd.metrics import metrics

    labels = {"target": np.array([0, 0, 1, 2, 2, 2]), "pred": np.array([0, 1, 1, 1]), "same": np.array([2, 2, 0, 2, 1, 0])}
    weights = {"pred": np.array([1.0, 2.0, 0.5, 0.5])}
    for w in (None, weights):
        got = metrics.js_of_states(labels, 4, "target", w)
        assert got == RK.js_of_states(labels, 4, "target", w) and got["target"] == 0.0 and got["same"] == 0.0 and got["pred"] > 0.0
    assert metrics.state_populations([0, 0, 1, -1, 3], 4).tolist() == [0.5, 0.25, 0.0, 0.25]
    assert metrics.state_populations([0, 1], 2, weights=[3.0, 1.0]).tolist() == [0.75, 0.25]
    assert RK.js(np.array([1.0, 0.0]), np.array([0.0, 1.0])) == pytest.approx(np.sqrt(np.log(2.0)))


def test_labels_equal_sklearn_lloyd_from_the_same_centres():
    cluster = pytest.importorskip("sklearn.cluster")
    x, blob = _planted()
    init = RK.farthest_points(x, 4)[1]
    km = cluster.KMeans(n_clusters=4, init=init, n_init=1, algorithm="lloyd", max_iter=100, tol=0.0).fit(x)
    res = RK.lloyd(x, init)
    assert np.array_equal(km.labels_, res["labels"]) and np.allclose(km.cluster_centers_, res["centres"], rtol=1e-12, atol=1e-12)


def test_the_cases_meet_their_preconditions():
    for T, d, k in KC.CASES:
        ref = KC.reference(T, d, k)
        assert ref["converged"] and ref["gap"] >= KC.MIN_GAP and ref["seed_gap"] >= KC.MIN_GAP
        print(f"(T, d, k) = {(T, d, k)}: {ref['n_iter']} iterations, assignment gap {ref['gap']:.2e}, seeding gap {ref['seed_gap']:.2e}")
    x, state = KC.three_basins()
    assert x.dtype == np.float32 and set(state.tolist()) == {0, 1, 2}


# ------------------------------------------------------------------------------------------------ header, binding, build
def test_every_kinetics_binding_has_the_arity_of_its_prototype():
    """The parser of test_host_cpu.py::test_every_binding_has_the_arity_of_its_prototype on include/str2str_kinetics.h."""
    from str2str_amd.ops import binding

    scalars = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
               "unsigned long long": ctypes.c_ulonglong}

    def ctype_of(param):
        decl = re.sub(r"\s+", " ", param.replace("*", " * ")).strip()
        if "*" in decl:
            return ctypes.c_char_p if decl.startswith("const char *") and decl.count("*") == 1 else ctypes.c_void_p
        return scalars[" ".join(w for w in decl.split(" ")[:-1] if w != "const")]

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "str2str_kinetics.h")).read(), flags=re.S)
    protos = {name: (ret, params) for ret, name, params in re.findall(r"^(int|long long)\s+(s2k_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)}
    assert set(protos) == set(binding._KINETICS_SIGNATURES) == set(binding.KINETICS_EXPORTS), sorted(set(protos) ^ set(binding._KINETICS_SIGNATURES))
    assert not set(binding.KINETICS_EXPORTS) & set(binding.EXPORTS) and all(n.startswith("s2k_") for n in binding.KINETICS_EXPORTS)
    for name, (ret, params) in protos.items():
        want = [] if params.strip() in ("", "void") else [ctype_of(p) for p in params.split(",")]
        assert want == binding._KINETICS_SIGNATURES[name], (name, want)
        assert ret == "int"
        if name != "s2k_abi_version":
            assert re.sub(r"\s+", " ", params.split(",")[-1]).strip() == "void* stream", name
    assert re.search(r"#define\s+S2K_ABI_VERSION\s+1\b", hdr) and binding.KINETICS_ABI_VERSION == 1 and binding.ABI_VERSION == 40
    for name, value in (("S2K_MAX_DIM", 64), ("S2K_MAX_CENTRES", 4096)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", hdr)


def test_the_unit_is_built_and_exported():
    from str2str_amd import build, ops

    assert build.UNITS["ensemble_kinetics.hip"] == ["-ffp-contract=off"] and os.path.isfile(os.path.join(build.CSRC, "ensemble_kinetics.hip"))
    if not os.path.exists(ops.LIB_PATH):
        build.build(verbose=False)
    lib = ops.load_library()
    for name in ops.KINETICS_EXPORTS:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert lib.s2k_abi_version() == ops.KINETICS_ABI_VERSION == 1
    assert (ops.KINETICS_MAX_DIM, ops.KINETICS_MAX_CENTRES) == (64, 4096)
    src = open(os.path.join(build.CSRC, "ensemble_kinetics.hip")).read()
    assert "wave_sum" in src and "launch_dynamic_lds" in src and "ensemble_common.h" in src      # the shared helpers, not copies of them


# ------------------------------------------------------------------------------------------------ argument errors, without a device
def test_wrappers_reject_bad_arguments_before_the_device():
    from str2str_amd import ops

    E = ops.HipLibraryError
    x, c = torch.zeros(5, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)
    lab = torch.zeros(5, dtype=torch.int32)
    for bad, match in ((lambda: ops.kmeans_assign(np.zeros((5, 3)), c), "expected tensors"), (lambda: ops.kmeans_assign(x[0], c), r"expected \[T, d\]"),
                       (lambda: ops.kmeans_assign(torch.zeros(5, 65, dtype=torch.float64), c), "at most 64"),
                       (lambda: ops.kmeans_assign(x, torch.zeros(2, 4, dtype=torch.float64)), "centres"),
                       (lambda: ops.kmeans_assign(x, torch.zeros(4097, 3, dtype=torch.float64)), "at most 4096"),
                       (lambda: ops.kmeans_assign(x, c, prev_labels=lab[:4]), "prev_labels"), (lambda: ops.kmeans_assign(x, c, max_centres=0), "max_centres"),
                       (lambda: ops.kmeans_update(x, lab[:4], c), "labels"), (lambda: ops.kmeans_update(x, lab, c[:, :2]), "centres"),
                       (lambda: ops.kmeans_update(x, lab, c, max_segments=0), "max_segments"),
                       (lambda: ops.farthest_points(x, 6), "6 centres out of 5"), (lambda: ops.farthest_points(x, 0), "k must be"),
                       (lambda: ops.farthest_points(x, 2, first=5), "first"), (lambda: ops.farthest_points(x, 2.5), "k must be"),
                       (lambda: ops.transition_counts(lab.reshape(5, 1), 2, 1), r"expected \[T\]"), (lambda: ops.transition_counts(lab, 0, 1), "n_states"),
                       (lambda: ops.transition_counts(lab, 2, 0), "lag"), (lambda: ops.transition_counts(lab, 2, 1, lengths=[5]), "lengths")):
        with pytest.raises(E, match=match):
            bad()
    # a good call gets as far as the device check: CPU tensors are refused, there is no fallback
    for good in (lambda: ops.kmeans_assign(x, c), lambda: ops.kmeans_update(x, lab, c), lambda: ops.farthest_points(x, 2),
                 lambda: ops.transition_counts(lab, 2, 1)):
        with pytest.raises(E, match="on the HIP device"):
            good()


def test_public_functions_reject_bad_arguments_before_the_device():
    from str2str_amd.metrics import metrics

    x = np.zeros((5, 3))
    for bad, match in ((lambda: metrics.kmeans(x, 0), "n_states"), (lambda: metrics.kmeans(x, 2.0), "n_states"), (lambda: metrics.kmeans(x, 2, max_iter=0), "max_iter"),
                       (lambda: metrics.kmeans(x, 2, init="random"), "init"), (lambda: metrics.kmeans(x[0], 2), r"\[T, d\]"),
                       (lambda: metrics.kmeans(np.zeros((5, 65)), 2), "at most 64"), (lambda: metrics.kmeans(x, 5000), "at most 4096"),
                       (lambda: metrics.msm(np.zeros(5, dtype=int), 0, 1), "n_states"), (lambda: metrics.msm(np.zeros(5, dtype=int), 2, 0), "lagtime"),
                       (lambda: metrics.msm(np.zeros((5, 1), dtype=int), 2, 1), r"\[T\]"),
                       (lambda: metrics.msm(np.zeros(5, dtype=int), 2, 1, lengths=[2, 2]), "lengths"),
                       (lambda: metrics.state_populations([0, 1], 2, weights=[1.0]), "weights"),
                       (lambda: metrics.assign_states(x[0], x), r"\[T, d\]")):
        with pytest.raises(ValueError, match=match):
            bad()
    assert list(inspect.signature(metrics.kmeans).parameters) == ["features", "n_states", "init", "first", "max_iter", "max_centres"]
    assert list(inspect.signature(metrics.msm).parameters) == ["labels", "n_states", "lagtime", "lengths", "reversible", "tol", "max_iter"]
    assert list(inspect.signature(metrics.js_msm).parameters) == ["ca_coords_dict", "ref_key", "lagtime", "n_states", "dim", "weights", "return_model"]
    assert metrics.EnsembleKMeans._fields == ("centres", "labels", "counts", "inertia", "n_iter", "converged")
    assert metrics.EnsembleMSM._fields == ("counts", "active", "transition_matrix", "stationary", "eigenvalues", "timescales", "lagtime", "converged")


# ------------------------------------------------------------------------------------------------ eval.py
def test_eval_msm_switch(monkeypatch):
    import eval as entry
    from str2str_amd.utils import config as C

    assert len(entry.REPORTS) == 5 and len(entry.EXTRA_METRICS) == 12 and "msm" not in [r.name for r in entry.REPORTS]
    assert entry.MSM_COLUMNS == ("js_msm", "n_active", "timescale_1", "timescale_2", "timescale_3")
    monkeypatch.setenv("TEST_DATA", "/nonexistent")
    compose = lambda *args: C.compose(os.path.join(ROOT, "configs"), "eval.yaml", list(args))   # noqa: E731
    assert entry.msm_switch(compose("+msm=true").get("msm")) is True and entry.msm_switch(compose("+msm=false").get("msm")) is False
    cfg = compose("+msm=true", "+msm_states=50", "+msm_lag=5")
    assert (cfg.get("msm_states"), cfg.get("msm_lag")) == (50, 5)
    assert compose().get("msm") is None and compose().get("msm_states") is None and compose().get("msm_lag") is None
    params = inspect.signature(entry.evaluate_prediction).parameters
    assert params["msm"].default is None and params["msm_states"].default is None and params["msm_lag"].default is None
    for value, want in ((None, False), (True, True), ("false", False), (" True ", True), ("0", False)):
        assert entry.msm_switch(value) is want
    for kw, match in ((dict(msm="maybe"), "msm"), (dict(msm_states=50), "needs msm=true"), (dict(msm=True, msm_states=0), "msm_states"),
                      (dict(msm=True, msm_lag=2.5), "msm_lag"), (dict(msm=True, msm_lag=True), "msm_lag")):
        with pytest.raises(ValueError, match=match):                               # rejected before anything is read or written
            entry.evaluate_prediction("/nonexistent/pred", "/nonexistent/target", **kw)
    assert entry.evaluate_prediction("/nonexistent/pred", "/nonexistent/target", msm=True, msm_states=50, msm_lag=5) == {}
