"""Clustering on the device (csrc/ensemble_cluster.hip) against the numpy yardstick of tests/ref_cluster.py.

Everything here is exact.  The integer-valued matrices make every comparison with the cutoff exact in float64; the end-to-end cases
threshold the very float64 values the already-tested matrix kernels produce (``pairwise_rmsd`` / ``pairwise_tm``), so the yardstick
sees the same booleans and no tolerance enters.  The planted ensemble additionally has to come back as its planted partition, which
holds only while no pair sits at the cutoff: the test checks that precondition with its own float64 SVD Kabsch.
"""
import functools
import glob

import numpy as np
import pytest
import torch

import ref_cluster as ref
from ensemble_cases import load_eval_entry

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = (1, 2, 63, 64, 65, 130, 257)      # word boundaries, a partial last word, several words
HIS = (3, 8, 40)
SIGMAS = (1e-3, 0.05, 0.5, 2.0, 8.0)


@functools.lru_cache(maxsize=None)
def integer_case(n, hi):
    """-> (d [n, n] float64, yardstick result on d <= 1)."""
    d = ref.integer_matrix(n, hi, 1000 * n + hi)
    d.setflags(write=False)
    return d, ref.gromos(d <= 1.0)


def _bits(adj):
    return adj.cpu().numpy().view(np.uint64)


def _same(got, want):
    for g, w, name in zip(got, want, ("labels", "centres", "sizes")):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == np.int32 and g.shape == w.shape and (g == w).all(), (name, g, w)


# ------------------------------------------------------------------------------------------------------------------------ adjacency
@pytest.mark.parametrize("n", SIZES)
def test_adjacency_bits_and_degrees(n):
    from str2str_amd import ops

    for hi in HIS:
        d = integer_case(n, hi)[0]
        v = torch.as_tensor(d).to(DEV)
        for at_least in (False, True):
            want = (d >= 1.0 if at_least else d <= 1.0) | np.eye(n, dtype=bool)
            adj, deg = ops.cluster_adjacency(v, 1.0, at_least)
            assert adj.shape == (n, -(-n // 64)) and adj.dtype == torch.int64 and deg.dtype == torch.int32
            assert (_bits(adj) == ref.pack_bits(want)).all()                      # padding bits included
            assert (deg.cpu().numpy() == want.sum(1)).all()
            adj7 = deg7 = None
            for r0 in range(0, n, 7):
                adj7, deg7 = ops.cluster_adjacency(v[r0:r0 + 7].contiguous(), 1.0, at_least, r0, adj7, deg7)
            assert torch.equal(adj7, adj) and torch.equal(deg7, deg)


def test_adjacency_nan_and_diagonal():
    from str2str_amd import ops

    n = 65
    d = integer_case(n, 3)[0].copy()
    d[2, 64] = d[64, 2] = np.nan
    d[np.arange(n), np.arange(n)] = 2.0                                            # twice the cutoff: the diagonal is set all the same
    for at_least in (False, True):
        with np.errstate(invalid="ignore"):
            want = (d >= 1.0 if at_least else d <= 1.0)
        want[np.arange(n), np.arange(n)] = True
        assert not want[2, 64] and not want[64, 2]
        adj, deg = ops.cluster_adjacency(torch.as_tensor(d).to(DEV), 1.0, at_least)
        assert (_bits(adj) == ref.pack_bits(want)).all() and (deg.cpu().numpy() == want.sum(1)).all()


def test_limits_and_argument_checks():
    from str2str_amd import ops

    v = torch.zeros(3, 5, dtype=torch.float64, device=DEV)
    with pytest.raises(ops.HipLibraryError):
        ops.cluster_adjacency(v, 1.0, row0=3)                                      # rows 3 .. 5 of a 5 x 5 matrix
    with pytest.raises(ops.HipLibraryError):
        ops.cluster_adjacency(v.float(), 1.0)
    with pytest.raises(ops.HipLibraryError):
        ops.cluster_adjacency(torch.zeros(1, ops.CLUSTER_MAX_N + 1, dtype=torch.float64, device=DEV), 1.0)
    adj, deg = ops.cluster_adjacency(torch.zeros(5, 5, dtype=torch.float64, device=DEV), 1.0)
    with pytest.raises(ops.HipLibraryError):
        ops.cluster_gromos(adj, deg[:4].contiguous())
    with pytest.raises(ops.HipLibraryError):
        ops.cluster_gromos(adj, deg, rounds_per_sync=0)


# ----------------------------------------------------------------------------------------------------------------------------- loop
@pytest.mark.parametrize("n", SIZES)
def test_loop_equals_the_yardstick(n):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    for hi in HIS:
        d, want = integer_case(n, hi)
        got = metrics.cluster_from_matrix(d, 1.0)
        assert isinstance(got, metrics.ClusterResult)
        _same(got, want)
        _same(metrics.cluster_from_matrix(torch.as_tensor(d).to(DEV), 1.0), want)  # a device tensor of one's own
        adj, deg = ops.cluster_adjacency(torch.as_tensor(d).to(DEV), 1.0)
        deg0 = deg.clone()
        for rounds in (1, 3, None):
            _same(ops.cluster_gromos(adj, deg) if rounds is None else ops.cluster_gromos(adj, deg, rounds_per_sync=rounds), want)
        assert torch.equal(deg, deg0)                                              # the caller's counts are left alone
        # similarities: the same relation read as 2 - d >= 1
        _same(metrics.cluster_from_matrix(2.0 - d, 1.0, at_least=True), want)


def test_all_and_none_adjacent():
    from str2str_amd.metrics import metrics

    n = 65
    labels, centres, sizes = metrics.cluster_from_matrix(np.zeros((n, n)), 1.0)
    assert centres.tolist() == [0] and sizes.tolist() == [n] and (labels == 0).all()
    far = np.full((n, n), 5.0)
    np.fill_diagonal(far, 0.0)
    labels, centres, sizes = metrics.cluster_from_matrix(far, 1.0)
    assert centres.tolist() == list(range(n)) and (sizes == 1).all() and labels.tolist() == list(range(n))


# ----------------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def planted():
    x, group = ref.planted_ensemble()
    x.setflags(write=False)
    return x, group


def test_cluster_rmsd_on_a_planted_ensemble():
    from str2str_amd.metrics import metrics

    x, group = planted()
    cutoff = 2.0
    got = metrics.cluster_rmsd(x, cutoff)
    # (a) the yardstick on the same float64 values
    _same(got, ref.gromos(metrics.pairwise_rmsd(x) <= cutoff))
    # (b) the planted partition; precondition: nothing at the cutoff, by this file's own float64 Kabsch
    r64 = ref.kabsch_rmsd_matrix(x)
    same = group[:, None] == group[None, :]
    print(f"planted: within <= {r64[same].max():.3f} A, between >= {r64[~same].min():.3f} A")
    assert np.abs(r64 - cutoff).min() > 1e-6
    assert r64[same].max() < cutoff < r64[~same].min()
    assert got.sizes.tolist() == [40, 25, 12, 3]
    assert (got.labels == group).all() and group[got.centres].tolist() == [0, 1, 2, 3]   # (the planted groups are in order of size)
    # (c) the chunking does not show
    _same(metrics.cluster_rmsd(x, cutoff, chunk_pairs=7 * 80), got)
    # (d) per-residue weights reach the matrix
    w = np.random.default_rng(5).uniform(0.5, 2.0, size=x.shape[1]).astype(np.float32)
    w[2::3] = 0.0
    for cut in (cutoff, 0.45):
        _same(metrics.cluster_rmsd(x, cut, weights=w), ref.gromos(metrics.pairwise_rmsd(x, weights=w) <= cut))


def test_cluster_tm_on_a_planted_ensemble():
    from str2str_amd.metrics import metrics

    x, _ = planted()
    got = metrics.cluster_tm(x, 0.5)
    _same(got, ref.gromos(metrics.pairwise_tm(x) >= 0.5))
    assert got.sizes.sum() == len(x) and len(got.centres) >= 4


def ragged_ensemble(rng, n, L):
    """The recipe of the RMSD tests: around one random walk, exact copies, copies with Gaussian noise of the SIGMAS, an unrelated chain
    and a mirror image in turn, each under a random rotation and a translation of up to 50 A per axis."""
    base, out = ref.random_walk(rng, L), []
    for s in range(n):
        kind = s % 8
        if kind == 0:
            y = base.copy()
        elif kind <= 5:
            y = base + rng.normal(size=base.shape) * SIGMAS[kind - 1]
        elif kind == 6:
            y = ref.random_walk(rng, L)
        else:
            y = base * np.array([-1.0, 1.0, 1.0])
        out.append(y @ ref.random_rotation(rng).T + rng.uniform(-50.0, 50.0, size=3))
    return np.asarray(out, dtype=np.float32)


@pytest.mark.parametrize("L", (1, 7, 35))
def test_cluster_rmsd_on_ragged_ensembles(L):
    from str2str_amd.metrics import metrics

    for R in (1, 17, 100):
        x = ragged_ensemble(np.random.default_rng(100 * L + R), R, L)
        got = metrics.cluster_rmsd(x, 1.0)
        _same(got, ref.gromos(metrics.pairwise_rmsd(x) <= 1.0))
        if L == 1:
            assert got.centres.tolist() == [0] and got.sizes.tolist() == [R]


# -------------------------------------------------------------------------------------------------------------------------- eval.py
def _atom37(ca):
    """CA traces [R, L, 3] -> atom37 [R, L, 37, 3] with N, CA and C placed (the writer leaves all-zero atoms out)."""
    a = np.zeros(ca.shape[:2] + (37, 3), dtype=np.float32)
    a[:, :, 1] = ca
    a[:, :, 0] = ca + np.float32([-0.5, 1.3, 0.2])
    a[:, :, 2] = ca + np.float32([1.4, 0.4, -0.3])
    return a


def _models(path):
    out = []
    for ln in open(path, "rb").read().split(b"\n"):
        if ln.startswith(b"MODEL"):
            out.append([])
        elif ln.startswith(b"ATOM"):
            out[-1].append(ln)
    return out


def test_eval_writes_cluster_centres_and_summary(tmp_path):
    from str2str_amd.common.pdb_utils import atom37_to_pdb, extract_backbone_coords
    from str2str_amd.metrics import metrics

    entry = load_eval_entry("s2s_eval_entry_cluster")
    x, _ = ref.planted_ensemble(seed=11, L=24, copies=(12, 7, 3, 1))
    target_dir = tmp_path / "targets"
    target_dir.mkdir()
    atom37_to_pdb(str(target_dir / "planted.pdb"), _atom37(ref.planted_ensemble(seed=12, L=24, copies=(25,))[0]))
    csvs = {}
    for sub, cutoff in (("plain", None), ("clustered", 2.0)):
        pred_dir = tmp_path / sub / "samples" / "all"
        pred_dir.mkdir(parents=True)
        pred_file = atom37_to_pdb(str(pred_dir / "planted.pdb"), _atom37(x))
        entry.evaluate_prediction(str(pred_dir), str(target_dir), tag="t", **({} if cutoff is None else {"cluster_cutoff": cutoff}))
        files = glob.glob(str(tmp_path / sub / "metrics_t_*.csv"))
        assert len(files) == 1
        csvs[sub] = open(files[0], "rb").read()
        out_pdb, out_csv = tmp_path / sub / "clusters" / "planted.pdb", glob.glob(str(tmp_path / sub / "clusters_t_*.csv"))
        if cutoff is None:
            assert not (tmp_path / sub / "clusters").exists() and not out_csv
            continue
        pred = extract_backbone_coords(pred_file)
        labels, centres, sizes = ref.gromos(metrics.pairwise_rmsd(pred) <= cutoff)
        assert sizes.tolist() == [12, 7, 3, 1]
        source, got = _models(pred_file), _models(str(out_pdb))
        assert len(got) == len(centres) and got == [source[c] for c in centres]          # the centres' own bytes, most populated first
        assert len(out_csv) == 1
        rows = [ln.rstrip("\n").split("\t") for ln in open(out_csv[0])]
        assert rows[0] == ["", "n_clusters", "top1_population", "top5_population", "n_singletons"] and len(rows) == 2
        assert rows[1][0] == "planted" and [float(v) for v in rows[1][1:]] == [4.0, round(12 / 23, 4), 1.0, 1.0]
    assert csvs["plain"] == csvs["clustered"]                                            # the metrics csv is untouched
