"""Time metrics.cluster_rmsd against the pairwise-RMSD walk it contains, alone, in the same process.

    python tools/cluster_timing.py [--out cluster_timing.json]

Cases: R = 10 000 structures at L = 35 and R = 1 000 at L = 256; 20 random-walk chains, every structure one of them with Gaussian noise of
0.2 .. 3.0 A under a random rigid motion, clustered at 3.0 A (tight copies form clusters, loose ones a singleton tail).  Host clock around
the whole call ending in a device synchronise, three timed repeats after a warm-up.  "walk" is the same row chunks of s2s_ca_rmsd_matrix
with the result dropped; the difference is thresholding plus the greedy loop.  One JSON line per case; profiles/cluster_timing.md is
written from them."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from str2str_amd import ops  # noqa: E402
from str2str_amd.metrics import metrics  # noqa: E402


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


def ensemble(R, L, n_base, seed):
    rng = np.random.default_rng(seed)
    bases = [random_walk(rng, L) for _ in range(n_base)]
    out = np.empty((R, L, 3), dtype=np.float32)
    for s in range(R):
        sigma = rng.uniform(0.2, 3.0)
        out[s] = (bases[s % n_base] + rng.normal(size=(L, 3)) * sigma) @ random_rotation(rng).T + rng.uniform(-50, 50, size=3)
    return out


def walk(x):
    n = x.shape[0]
    rows = ops.rmsd_row_chunk(n, metrics.COVERAGE_CHUNK_PAIRS)
    for r0 in range(0, n, rows):
        ops.ca_rmsd_matrix(x[r0:r0 + rows], x)


def timed(fn, repeats=3):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


results = []
for R, L, cutoff in ((10000, 35, 3.0), (1000, 256, 3.0)):
    x = metrics._dev(ensemble(R, L, 20, R + L))
    res = metrics.cluster_rmsd(x, cutoff)
    t_walk = timed(lambda: walk(x))
    t_clu = timed(lambda: metrics.cluster_rmsd(x, cutoff))
    row = {"R": R, "L": L, "cutoff": cutoff, "n_clusters": int(len(res.sizes)), "n_singletons": int((res.sizes == 1).sum()),
           "top_sizes": res.sizes[:5].tolist(), "walk_s": t_walk, "cluster_rmsd_s": t_clu,
           "ratio_median": float(np.median(t_clu) / np.median(t_walk))}
    print(json.dumps(row), flush=True)
    results.append(row)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
