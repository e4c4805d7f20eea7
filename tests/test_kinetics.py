"""The kinetics family on the device (include/str2str_kinetics.h) against tests/ref_kinetics.py on the cases of tests/kinetics_cases.py.

Integers -- labels, seeding indices, counts, iteration counts -- must be the restatement's: the cases' preconditions (kinetics_cases.reference)
keep every deciding comparison at least 1e-9 relative away from a tie.  Floating-point results have a-priori bounds:
  dist2     the device adds d terms (x_i - c_i)^2 in the restatement's order; allowing each of the d - 1 additions, the difference and the
            square one rounding of their own in either computation gives (d + 16) 2^-52 times the sum of the magnitudes
            sum_i (|x_i| + |c_i|)^2 with room to spare.
  centres   a sum of n_j terms in any order is within (n_j - 1) 2^-52 sum |x_t| of the exact sum, the restatement's fsum is exact to one
            rounding, the division adds one: (n_j + 16) 2^-52 sum_t |x_t| / n_j.
Everything else is byte equality: between tile bounds, workspace sizes and repeated calls."""
import glob
import os

import numpy as np
import pytest
import torch

import kinetics_cases as KC
import ref_kinetics as RK
from conftest import GOLDEN, record_margin
from ensemble_cases import load_eval_entry, write_models
from guarded_alloc import same_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 2.0 ** -52
CASE_IDS = ["-".join(map(str, c)) for c in KC.CASES]


def dev(a, dtype=None):
    return torch.as_tensor(np.array(a)).to(DEV, dtype).contiguous()          # (a copy: the cases' arrays are read-only)


@pytest.mark.parametrize("case", KC.CASES, ids=CASE_IDS)
def test_assign(case):
    from str2str_amd import ops

    T, d, k = case
    ref = KC.reference(*case)
    x = dev(ref["x"])
    for name, centres in (("seeds", ref["seed_centres"]), ("final", ref["centres"])):
        want, want_d2, gap = RK.assign(ref["x"], centres)
        assert gap >= KC.MIN_GAP
        c = dev(centres)
        labels, dist2, changed = ops.kmeans_assign(x, c)
        assert changed is None and labels.dtype == torch.int32 and dist2.dtype == torch.float64
        assert np.array_equal(labels.cpu().numpy(), want), name
        mag = (np.abs(ref["x"]) + np.abs(centres[want])) ** 2
        err, bound = np.abs(dist2.cpu().numpy() - want_d2), (d + 16) * EPS * mag.sum(1)
        print(f"{case} {name}: dist2 error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        record_margin(f"kinetics assign dist2 (T, d, k) = {case}: error / bound", float((err / np.maximum(bound, 1e-300)).max()), 1.0)
        assert (err <= bound).all()
        for tile in sorted({1, 7, k}):                              # the tile bound changes no byte
            l2, d2, _ = ops.kmeans_assign(x, c, max_centres=tile)
            assert same_bytes(l2, labels) and same_bytes(d2, dist2), (name, tile)
        # the changed-label counter: against the other labels of the case, against the labels themselves, against all-unassigned
        other = ref["labels"] if name == "seeds" else RK.assign(ref["x"], ref["seed_centres"])[0]
        for prev, n in ((other, int((other != want).sum())), (want, 0), (np.full(T, -1, dtype=np.int32), T)):
            l3, d3, changed = ops.kmeans_assign(x, c, prev_labels=dev(prev, torch.int32))
            assert changed.tolist() == [n] and same_bytes(l3, labels) and same_bytes(d3, dist2)


@pytest.mark.parametrize("case", KC.CASES, ids=CASE_IDS)
def test_centre_update(case):
    from str2str_amd import ops

    T, d, k = case
    ref = KC.reference(*case)
    labels = RK.assign(ref["x"], ref["seed_centres"])[0].copy()
    if T > 64:
        labels[T // 3] = -1                                         # an unassigned frame belongs to no cluster
    # cluster k has no member: its centre, of awkward bytes, must come back untouched
    start = np.concatenate([ref["seed_centres"], np.full((1, d), -7.0 / 3.0)])
    counts, want, mags = RK.update(ref["x"], labels, start)
    x, lab = dev(ref["x"]), dev(labels, torch.int32)

    def run(**kw):
        c = dev(start)
        n = ops.kmeans_update(x, lab, c, **kw)
        return n, c

    n, c = run()
    assert n.dtype == torch.int32 and n.tolist() == counts.tolist() and counts[k] == 0 and counts.sum() == T - (T > 64)
    assert c[k].cpu().numpy().tobytes() == start[k].tobytes()
    err = np.abs(c.cpu().numpy() - want)[:k]
    bound = ((counts[:k, None] + 16) * EPS * mags[:k] / np.maximum(counts[:k, None], 1))
    assert (counts[:k] > 0).all()
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{case}: centre error / bound = {ratio:.3f}")
    record_margin(f"kinetics centre update (T, d, k) = {case}: error / bound", ratio, 1.0)
    assert (err <= bound).all()
    for kw in ({}, {"max_segments": 1}, {"max_segments": 3}):       # a repeated call and two more workspace sizes: the same bytes
        n2, c2 = run(**kw)
        assert same_bytes(n2, n) and same_bytes(c2, c), kw


@pytest.mark.parametrize("case", KC.CASES, ids=CASE_IDS)
def test_farthest_point(case):
    from str2str_amd import ops

    T, d, k = case
    ref = KC.reference(*case)
    x = dev(ref["x"])
    indices, centres = ops.farthest_points(x, k)
    assert indices.dtype == torch.int32 and indices.tolist() == ref["seed_indices"].tolist()
    assert centres.cpu().numpy().tobytes() == ref["seed_centres"].tobytes()
    if T > 1:                                                       # another first frame: another greedy sequence, the restatement's
        first = T - 1
        want = RK.farthest_points(ref["x"], min(k, 5), first)
        assert want[2] >= KC.MIN_GAP
        got = ops.farthest_points(x, min(k, 5), first=first)
        assert got[0].tolist() == want[0].tolist() and got[0][0] == first


@pytest.mark.parametrize("case", KC.CASES, ids=CASE_IDS)
def test_kmeans(case):
    from str2str_amd.metrics import metrics

    T, d, k = case
    ref = KC.reference(*case)
    res = metrics.kmeans(ref["x"], k)
    assert np.array_equal(res.labels, ref["labels"]) and res.labels.dtype == np.int32
    assert (res.n_iter, res.converged) == (ref["n_iter"], True) and res.counts.tolist() == ref["counts"].tolist()
    # (every centre is a mean of at most T frames: the bound of the update at its loosest, n_j = T and |x| = max |x|)
    assert np.abs(res.centres - ref["centres"]).max() <= (T + 16) * EPS * np.abs(ref["x"]).max()
    assert res.inertia == pytest.approx(ref["inertia"], rel=1e-12)
    assert np.array_equal(metrics.assign_states(ref["x"], res), res.labels)
    assert np.array_equal(metrics.assign_states(torch.as_tensor(ref["x"]), res.centres), res.labels)
    tiled = metrics.kmeans(ref["x"], k, init=ref["seed_centres"], max_centres=7)        # the seeds as an array, a tile bound: no bit changes
    assert np.array_equal(tiled.labels, res.labels) and tiled.centres.tobytes() == res.centres.tobytes() and tiled.n_iter == res.n_iter


def test_kmeans_stops_at_max_iter():
    from str2str_amd.metrics import metrics

    case = (4099, 4, 40)
    ref = KC.reference(*case)
    assert ref["n_iter"] > 4
    cut = RK.lloyd(ref["x"], ref["seed_centres"], max_iter=3)
    res = metrics.kmeans(ref["x"], case[2], max_iter=3)
    assert (res.n_iter, res.converged) == (3, False) == (cut["n_iter"], cut["converged"])
    assert np.array_equal(res.labels, cut["labels"]) and np.abs(res.centres - cut["centres"]).max() <= (case[0] + 16) * EPS * np.abs(ref["x"]).max()
    assert not np.array_equal(res.labels, ref["labels"])
    # the returned labels are the assignment against the returned centres
    assert np.array_equal(RK.assign(ref["x"], res.centres)[0], res.labels)
    one = metrics.kmeans(ref["x"], case[2], max_iter=1)
    assert (one.n_iter, one.converged) == (1, False) and one.centres.tobytes() == ref["seed_centres"].tobytes()


@pytest.mark.parametrize("n_traj", (1, 3))
@pytest.mark.parametrize("shape", KC.COUNT_CASES, ids=["-".join(map(str, c)) for c in KC.COUNT_CASES])
def test_transition_counts(shape, n_traj):
    from str2str_amd import ops

    T, k, lag = shape
    labels = KC.label_string(T, k)
    lengths = KC.split_lengths(T, n_traj)
    want = RK.transition_counts(labels, k, lag, lengths)
    got = ops.transition_counts(dev(labels, torch.int32), k, lag, None if n_traj == 1 else dev(np.asarray(lengths), torch.int32))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.as_tensor(want))
    if T > 1:
        assert want.sum() > 0 and (n_traj == 1 or want.sum() < RK.transition_counts(labels, k, lag).sum())
    again = ops.transition_counts(dev(labels, torch.int32), k, lag, dev(np.asarray(lengths), torch.int32))
    assert torch.equal(again, got)


# ------------------------------------------------------------------------------------------------ msm, js_msm, eval.py
N_STATES, LAG = 6, 5


@pytest.fixture(scope="module")
def basins():
    """The planted trajectory as the target, a sample that avoids the third well, and the restated pipeline on them."""
    from str2str_amd.metrics import metrics

    target, state = KC.three_basins()
    rng = np.random.default_rng(8)
    pick = rng.permutation(np.flatnonzero(state != 2))[:300]
    feats = {"target": target, "pred": target[pick] + 0.01 * rng.standard_normal((300, 2)).astype(np.float32)}
    model = metrics.tica(target, LAG, dim=4)
    proj = {key: metrics.tica_project(v, model) for key, v in feats.items()}
    km = RK.kmeans(proj["target"], N_STATES)
    assert km["converged"] and km["gap"] >= KC.MIN_GAP and RK.farthest_points(proj["target"], N_STATES)[2] >= KC.MIN_GAP
    labels = {key: RK.assign(p, km["centres"]) for key, p in proj.items()}
    assert min(v[2] for v in labels.values()) >= KC.MIN_GAP
    return dict(feats=feats, state=state, proj=proj, km=km, labels={key: v[0] for key, v in labels.items()})


def test_msm(basins):
    from str2str_amd.metrics import metrics

    labels = basins["labels"]["target"]
    counts = RK.transition_counts(labels, N_STATES, LAG)
    want = RK.msm(counts, LAG)
    got = metrics.msm(labels, N_STATES, LAG)
    assert np.array_equal(got.counts, counts) and got.counts.dtype == np.int64 and got.counts.sum() == len(labels) - LAG
    assert got.active.tolist() == want["active"].tolist() and got.converged and got.lagtime == LAG
    # the margin: the restatement at tol = 1e-15 in np.longdouble against itself at tol = 1e-12 in float64, times 4
    act = want["active"]
    t_ld, pi_ld, ok, _ = RK.reversible_mle(counts[np.ix_(act, act)], tol=1e-15, dtype=np.longdouble)
    assert ok
    root = np.sqrt(pi_ld)
    sym = (root[:, None] * t_ld / root[None, :]).astype(np.float64)
    lam = np.linalg.eigvalsh(0.5 * (sym + sym.T))
    mag = np.sort(np.abs(lam))[::-1][1:]
    ts_ld = np.abs(-LAG / np.log(mag))
    for name, fine in (("transition_matrix", t_ld), ("stationary", pi_ld), ("timescales", ts_ld)):
        measured = float(np.abs(want[name] - fine).max())
        err = float(np.abs(getattr(got, name) - want[name]).max())
        print(f"msm {name}: |device pipeline - restatement| = {err:.3e}, measured longdouble distance {measured:.3e}")
        record_margin(f"MSM three basins, {name}: error (absolute)", err, 4.0 * measured)
        assert measured > 0.0 and err <= 4.0 * measured, name
    # what the planted chain says: three metastable wells -> two slow processes, far above the lag; the rest decays within it
    assert len(got.timescales) == len(act) - 1 and got.timescales[1] > 4 * LAG and (got.timescales[2:] < LAG).all()
    assert abs(got.stationary.sum() - 1.0) < 1e-12 and np.abs(got.transition_matrix.sum(1) - 1.0).max() < 1e-12
    plain = metrics.msm(labels, N_STATES, LAG, reversible=False)
    assert np.allclose(plain.transition_matrix, RK.row_normalised(counts[np.ix_(act, act)]), rtol=1e-14, atol=0)
    # two trajectories: the pairs across the cut are gone
    halves = metrics.msm(labels, N_STATES, LAG, lengths=[700, len(labels) - 700])
    assert np.array_equal(halves.counts, RK.transition_counts(labels, N_STATES, LAG, [700, len(labels) - 700])) and halves.counts.sum() == len(labels) - 2 * LAG


def test_js_msm(basins):
    from str2str_amd.metrics import metrics

    feats, labels = basins["feats"], basins["labels"]
    want = RK.js_of_states(labels, N_STATES)
    got, model = metrics.js_msm(feats, ref_key="target", lagtime=LAG, n_states=N_STATES, return_model=True)
    assert got == want and got["target"] == 0.0 and 0.1 < got["pred"] <= 1.0 and list(got) == ["pred", "target"]
    assert np.array_equal(model.counts, RK.transition_counts(labels["target"], N_STATES, LAG))
    assert metrics.js_msm(feats, lagtime=LAG, n_states=N_STATES) == want
    w = {"pred": np.linspace(0.5, 2.0, len(feats["pred"]))}
    assert metrics.js_msm(feats, lagtime=LAG, n_states=N_STATES, weights=w) == RK.js_of_states(labels, N_STATES, weights=w) != want
    assert metrics.js_msm({"target": feats["target"], "same": feats["target"]}, lagtime=LAG, n_states=N_STATES)["same"] == 0.0
    km = metrics.kmeans(basins["proj"]["target"], N_STATES)
    assert np.array_equal(km.labels, basins["km"]["labels"]) and km.n_iter == basins["km"]["n_iter"]
    # the states see the wells: every microstate lies in one planted well
    assert all(len(set(basins["state"][labels["target"] == j].tolist())) == 1 for j in range(N_STATES))
    with pytest.raises(ValueError, match="frames are not enough"):
        metrics.js_msm({"target": feats["target"][:LAG], "pred": feats["pred"]}, lagtime=LAG, n_states=2)
    with pytest.raises(ValueError, match="states out of"):
        metrics.js_msm({"target": feats["target"][:8], "pred": feats["pred"]}, lagtime=LAG, n_states=9)


def test_eval_msm_switch(tmp_path, basins):
    """CLN025 moved by the planted three-basin coordinates (the chain's second half along x, its last three residues along y) as a target
    trajectory of 600 frames, 80 samples from two of the wells.  ``msm=True`` adds msm_t_*.csv and msm/CLN025.csv and leaves the metrics csv
    as it is without it; a target shorter than the lag leaves NaN."""
    from str2str_amd.common.pdb_utils import extract_backbone_coords
    from str2str_amd.metrics import metrics

    entry = load_eval_entry("s2s_eval_entry_msm")
    fixture = os.path.join(GOLDEN, "pdb", "CLN025.pdb")
    base = extract_backbone_coords(fixture)[0]
    L = base.shape[0]
    rng = np.random.default_rng(21)

    def structures(f):
        x = base[None] + rng.normal(size=(len(f), L, 3)) * 0.2
        x[:, L // 2:, 0] += f[:, :1]
        x[:, -3:, 1] += f[:, 1:]
        return x

    target_dir = tmp_path / "targets"
    target_dir.mkdir()
    write_models(str(target_dir / "CLN025.pdb"), fixture, structures(basins["feats"]["target"][:600].astype(np.float64)))
    samples = structures(basins["feats"]["pred"][:80].astype(np.float64))
    rows = {}
    for sub, kw in (("off", {}), ("on", dict(msm=True, msm_states=N_STATES, msm_lag=LAG)), ("short", dict(msm="true", msm_lag=700))):
        pred_dir = tmp_path / sub / "samples" / "all"
        pred_dir.mkdir(parents=True)
        write_models(str(pred_dir / "CLN025.pdb"), fixture, samples)
        entry.evaluate_prediction(str(pred_dir), str(target_dir), tag="t", **kw)
        rows[sub] = [ln.rstrip("\n").split("\t") for ln in open(glob.glob(str(tmp_path / sub / "metrics_t_*.csv"))[0])]
    assert sorted(f.split("_")[0] for f in os.listdir(tmp_path / "off")) == ["metrics", "samples"]
    assert sorted(f.split("_")[0] for f in os.listdir(tmp_path / "on")) == ["metrics", "msm", "msm", "samples"]
    assert rows["on"] == rows["off"]
    summary = [ln.rstrip("\n").split("\t") for ln in open(glob.glob(str(tmp_path / "on" / "msm_t_*.csv"))[0])]
    assert summary[0] == [""] + list(entry.MSM_COLUMNS) and [r[0] for r in summary[1:]] == ["CLN025"]
    ca = {"target": extract_backbone_coords(str(target_dir / "CLN025.pdb")), "pred": extract_backbone_coords(str(tmp_path / "on" / "samples" / "all" / "CLN025.pdb"))}
    want, model = metrics.js_msm(ca, lagtime=LAG, n_states=N_STATES, return_model=True)
    row = dict(zip(summary[0][1:], summary[1][1:]))
    assert float(row["js_msm"]) == want["pred"] > 0.0 and int(row["n_active"]) == len(model.active) >= 3
    assert [float(row[f"timescale_{i + 1}"]) for i in range(3)] == pytest.approx(list(model.timescales[:3]), rel=1e-9)
    table = [ln.rstrip("\n").split("\t") for ln in open(tmp_path / "on" / "msm" / "CLN025.csv")]
    assert table[0] == ["state", "population_target", "population_pred", "stationary_target"] and len(table) == 1 + N_STATES
    cols = np.array([[float(v) if v else np.nan for v in r] for r in table[1:]])
    assert cols[:, 0].tolist() == list(range(N_STATES)) and cols[:, 1].sum() == pytest.approx(1.0) and cols[:, 2].sum() == pytest.approx(1.0)
    assert np.nansum(cols[:, 3]) == pytest.approx(1.0) and np.allclose(cols[model.active, 3], model.stationary, rtol=1e-9)
    short = [ln.rstrip("\n").split("\t") for ln in open(glob.glob(str(tmp_path / "short" / "msm_t_*.csv"))[0])]
    assert short[1][0] == "CLN025" and all(v == "" for v in short[1][1:])            # NaN cells: the target has fewer frames than the lag
