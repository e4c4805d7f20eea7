"""Clustering without a GPU: the numpy yardstick of tests/ref_cluster.py on hand cases and its defining properties, the host side of the
feature (MODEL selection, argument checks that must come before any device call), and the coverage the device test cases claim."""
import os

import numpy as np
import pytest

import ref_cluster as ref
from conftest import GOLDEN, ROOT
from ensemble_cases import load_eval_entry

SIZES = (1, 2, 63, 64, 65, 130, 257)
HIS = (3, 8, 40)


def test_yardstick_on_hand_cases():
    path = np.abs(np.subtract.outer(np.arange(5), np.arange(5))) <= 1      # neighbour counts with self: 3, 4, 4, 4, 3 -> vertex 1 first
    labels, centres, sizes = ref.gromos(path)
    assert centres.tolist() == [1, 3] and sizes.tolist() == [3, 2] and labels.tolist() == [0, 0, 0, 1, 1]
    labels, centres, sizes = ref.gromos(np.ones((9, 9), dtype=bool))
    assert centres.tolist() == [0] and sizes.tolist() == [9] and (labels == 0).all()
    labels, centres, sizes = ref.gromos(np.zeros((9, 9), dtype=bool))
    assert centres.tolist() == list(range(9)) and (sizes == 1).all() and labels.tolist() == list(range(9))
    assert all(a.dtype == np.int32 for a in (labels, centres, sizes))


@pytest.mark.parametrize("n,p", [(1, 0.5), (17, 0.1), (64, 0.05), (130, 0.02), (200, 0.3)])
def test_yardstick_properties_on_random_graphs(n, p):
    rng = np.random.default_rng(100 + n)
    upper = np.triu(rng.random((n, n)) < p, 1)
    adj = upper | upper.T
    labels, centres, sizes = ref.gromos(adj)
    K = len(centres)
    assert labels.min() == 0 and labels.max() == K - 1 and sizes.sum() == n          # a partition ...
    assert (np.bincount(labels, minlength=K) == sizes).all() and (sizes >= 1).all()  # ... whose parts have the stated sizes
    assert (np.diff(sizes) <= 0).all()                                               # live counts only fall
    assert (labels[centres] == np.arange(K)).all()
    assert ((adj | np.eye(n, dtype=bool))[centres[labels], np.arange(n)]).all()      # every member is adjacent to its centre


def test_bit_packing_layout():
    adj = np.zeros((3, 70), dtype=bool)
    adj[0, 0] = adj[1, 63] = adj[2, 64] = adj[2, 69] = True
    words = ref.pack_bits(adj)
    assert words.dtype == np.uint64 and words.shape == (3, 2)
    assert words.tolist() == [[1, 0], [1 << 63, 0], [0, 1 | (1 << 5)]]


def test_device_cases_cover_ties_tails_and_word_edges():
    """What the integer matrices of tests/test_ensemble_cluster.py exercise, stated by the yardstick: several clusters, a tie at the top
    count (the tie-break) and a tail of at least two singletons (the shortcut), each in some case."""
    ties = tails = 0
    counts = []
    for n in SIZES:
        for hi in HIS:
            adj = ref.integer_matrix(n, hi, 1000 * n + hi) <= 1.0
            labels, centres, sizes = ref.gromos(adj)
            counts.append(len(centres))
            deg = (adj | np.eye(n, dtype=bool)).sum(1)
            ties += int((deg == deg.max()).sum() > 1)
            tails += int((sizes == 1).sum() >= 2)
    assert min(counts) == 1 and max(counts) > 10 and ties >= 3 and tails >= 3, (counts, ties, tails)


def test_select_pdb_models_swaps_and_rejects(tmp_path):
    from str2str_amd.common.pdb_utils import select_pdb_models

    src = os.path.join(GOLDEN, "io_atom37_two_models.pdb.txt")

    def models(path):
        out, cur = [], None
        for ln in open(path, "rb").read().split(b"\n"):
            if ln.startswith(b"MODEL"):
                cur = []
                out.append((ln, cur))
            elif ln.startswith((b"ATOM", b"TER")):
                cur.append(ln)
        return out

    want = models(src)
    assert len(want) == 2 and want[0][1] != want[1][1]
    dst = select_pdb_models(src, [1, 0], str(tmp_path / "sub" / "swapped.pdb"))
    got = models(dst)
    assert [m[1] for m in got] == [want[1][1], want[0][1]]                              # the source's own record bytes
    assert [m[0].split() for m in got] == [[b"MODEL", b"1"], [b"MODEL", b"2"]]          # renumbered
    select_pdb_models(src, [0, 1], str(tmp_path / "same.pdb"))
    assert open(tmp_path / "same.pdb", "rb").read() == open(src, "rb").read()
    select_pdb_models(src, [1], str(tmp_path / "one.pdb"))
    assert [m[1] for m in models(str(tmp_path / "one.pdb"))] == [want[1][1]]
    for bad in ([2], [0, -1]):
        with pytest.raises(IndexError):
            select_pdb_models(src, bad, str(tmp_path / "bad.pdb"))


def _no_device(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("touched the device"))  # noqa: E731
    monkeypatch.setattr(metrics, "_dev", boom)
    for name in ("cluster_adjacency", "cluster_gromos", "ca_rmsd_matrix", "ca_tm_matrix"):
        monkeypatch.setattr(ops, name, boom)
    return metrics


def test_cutoffs_are_checked_before_the_device(monkeypatch):
    metrics = _no_device(monkeypatch)
    x = np.zeros((4, 5, 3), dtype=np.float32)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            metrics.cluster_rmsd(x, bad)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            metrics.cluster_tm(x, bad)


def test_asymmetric_matrix_is_rejected_before_the_device(monkeypatch):
    metrics = _no_device(monkeypatch)
    m = ref.integer_matrix(9, 3, 0)
    m[2, 5] += 1.0
    with pytest.raises(ValueError):
        metrics.cluster_from_matrix(m, 1.0)
    with pytest.raises(ValueError):
        metrics.cluster_from_matrix(np.zeros((3, 4)), 1.0)


def test_abi_and_interface_are_declared():
    import re

    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "str2str_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"^int\s+(s2s_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M))
    for name in ("s2s_cluster_adjacency", "s2s_cluster_gromos"):
        assert name in protos and name in ops.EXPORTS and "void* stream" in protos[name]
        assert protos[name].count(",") + 1 == len(ops.binding._SIGNATURES[name])
    assert ops.ABI_VERSION >= 36 and callable(ops.cluster_adjacency) and callable(ops.cluster_gromos)
    assert metrics.ClusterResult._fields == ("labels", "centres", "sizes")


def test_cluster_cutoff_parses_from_the_command_line(monkeypatch):

    from str2str_amd.utils import config as C

    monkeypatch.setenv("TEST_DATA", "/nonexistent")
    cfg = C.compose(os.path.join(ROOT, "configs"), "eval.yaml", ["+cluster_cutoff=2.5"])
    assert float(cfg.get("cluster_cutoff")) == 2.5
    assert C.compose(os.path.join(ROOT, "configs"), "eval.yaml", []).get("cluster_cutoff") is None
    entry = load_eval_entry("s2s_eval_entry_cluster_cpu")
    row = entry.cluster_summary([40, 25, 12, 3, 1, 1])
    assert row == {"n_clusters": 6, "top1_population": 0.4878, "top5_population": 0.9878, "n_singletons": 2}
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            entry.evaluate_prediction("/nonexistent", os.path.join(GOLDEN, "pdb"), tag="t", cluster_cutoff=bad)
