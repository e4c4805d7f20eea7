"""Time the Markov-state-model path (metrics.kmeans / metrics.msm) split into its device parts, next to scikit-learn's Lloyd on the host.

    python tools/kinetics_timing.py [--out profiles/msm_timing.md]     all cases, each in a child process under its own time limit
    python tools/kinetics_timing.py --case msm_100000_k100             one case, one JSON line

Cases: T = 100 000 and 1 000 000 feature rows of d = 4 (what a TICA projection gives), k = 100 and 1000 states.  The rows are Gaussian blobs of
unit width around k // 2 centres of spread 6, seeded.  Timed, each of three repetitions between its own pair of device events after one
warm-up: the seeding (s2k_farthest_point: 2 k launches), one assignment (s2k_assign), one update (s2k_centre_update: count, scan, fill,
sum) and the transition counts at lag 20 (s2k_transition_counts).  Timed with the wall clock around a device synchronise, three
repetitions: the whole metrics.kmeans from given centres, MAX_ITER assignments at the most, with its readback of the changed-label counter per
iteration and the copies of its results.  Beside it, once, sklearn.cluster.KMeans(init=<the same centres>, n_init=1, algorithm="lloyd",
max_iter=<the same>, tol=0) on the host's cores, where scikit-learn is installed.  There is no pass/fail condition: the report records what
the run gives."""
import os
import sys
import time

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

D, LAG, MAX_ITER, REPEATS = 4, 20, 10, 3
CASES = {f"msm_{T}_k{k}": (T, k) for T in (100000, 1000000) for k in (100, 1000)}
CASE_TIMEOUT_S = 900


def run_case(name):
    import numpy as np
    import torch

    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    T, k = CASES[name]
    rng = np.random.default_rng([T, k])
    blob = 6.0 * rng.standard_normal((k // 2, D))
    host = blob[rng.integers(0, len(blob), size=T)] + rng.standard_normal((T, D))
    x = torch.as_tensor(host).to("cuda").contiguous()
    seed_ms = timing_common.time_repetitions(lambda: ops.farthest_points(x, k), REPEATS, warmup=1)
    centres = ops.farthest_points(x, k)[1]
    assign_ms = timing_common.time_repetitions(lambda: ops.kmeans_assign(x, centres), REPEATS, warmup=1)
    labels = ops.kmeans_assign(x, centres)[0]
    scratch = centres.clone()
    update_ms = timing_common.time_repetitions(lambda: ops.kmeans_update(x, labels, scratch), REPEATS, warmup=1)
    counts_ms = timing_common.time_repetitions(lambda: ops.transition_counts(labels, k, LAG), REPEATS, warmup=1)
    init = centres.cpu().numpy()
    metrics.kmeans(x, k, init=init, max_iter=2)                       # warm-up
    kmeans_s = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = metrics.kmeans(x, k, init=init, max_iter=MAX_ITER)
        torch.cuda.synchronize()
        kmeans_s.append(time.perf_counter() - t0)
    out = {"case": name, "T": T, "k": k, "d": D, "device": torch.cuda.get_device_name(0), "seed_ms": seed_ms, "assign_ms": assign_ms,
           "update_ms": update_ms, "counts_ms": counts_ms, "kmeans_s": kmeans_s, "n_iter": res.n_iter, "converged": res.converged,
           "sklearn_s": None, "sklearn_iter": None, "labels_equal": None, "threads": os.cpu_count() if "OMP_NUM_THREADS" not in os.environ
           else int(os.environ["OMP_NUM_THREADS"])}
    try:
        from sklearn.cluster import KMeans
    except ImportError:
        return out
    t0 = time.perf_counter()
    km = KMeans(n_clusters=k, init=init, n_init=1, algorithm="lloyd", max_iter=MAX_ITER, tol=0.0).fit(host)
    out.update(sklearn_s=time.perf_counter() - t0, sklearn_iter=int(km.n_iter_), labels_equal=float((km.labels_ == res.labels).mean()))
    return out


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "msm_timing.md"), CASE_TIMEOUT_S)
    if rows is None:
        return 0
    ms = lambda ts: ", ".join(f"{t:.3f}" for t in ts)   # noqa: E731
    lines = ["# Markov state models: k-means and transition counts on the device", "",
             f"Device: {rows[0]['device']}.  `python tools/kinetics_timing.py`; every repetition of a device part between its own pair of device "
             f"events, after one warm-up; the whole `metrics.kmeans` (given centres, at most {MAX_ITER} assignments, with its per-iteration readback "
             "and the copies of its results) with the wall clock around a device synchronise; scikit-learn once with the wall clock (all "
             f"measured).  d = {D}, lag {LAG}.  Inputs: Gaussian blobs of unit width around k // 2 centres of spread 6.  No pass/fail condition: this "
             "is the record of one run.  scikit-learn runs `max_iter` assign-and-update steps and then one more assignment, `metrics.kmeans` "
             "`max_iter` assignments in all, and scikit-learn relocates empty clusters: where neither has converged the last column compares "
             "labels one assignment apart and is not an equality check (`tests/test_kinetics_cpu.py` has one, on a case that converges).", "",
             "| case | seeding, 2k launches (ms) | one assignment (ms) | one update (ms) | transition counts (ms) | whole kmeans (s) | assignments "
             "run | sklearn Lloyd, same centres and max_iter (s) | its iterations | host threads | labels equal to sklearn's |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        sk = "not installed" if r["sklearn_s"] is None else f"{r['sklearn_s']:.2f}"
        eq = "-" if r["labels_equal"] is None else f"{r['labels_equal']:.6f}"
        lines.append(f"| {r['case']} | {ms(r['seed_ms'])} | {ms(r['assign_ms'])} | {ms(r['update_ms'])} | {ms(r['counts_ms'])} | "
                     f"{', '.join(f'{t:.3f}' for t in r['kmeans_s'])} | {r['n_iter']} | {sk} | {r['sklearn_iter'] or '-'} | {r['threads']} | {eq} |")
    lines += ["", "Derived from the measured times: what one assignment sustains (T k d differences, squares and additions: 3 T k d float64 "
              "operations) and the seeding's time per launch.", "",
              "| case | assignment: float64 operations / s | seeding: time per launch (us) | whole kmeans against sklearn |", "|---|---|---|---|"]
    for r in rows:
        ratio = "-" if r["sklearn_s"] is None else f"{r['sklearn_s'] / min(r['kmeans_s']):.1f} x"
        lines.append(f"| {r['case']} | {3.0 * r['T'] * r['k'] * r['d'] / (min(r['assign_ms']) * 1e-3):.3e} | "
                     f"{min(r['seed_ms']) * 1e3 / (2 * r['k']):.1f} | {ratio} |")
    lines.append("")
    timing_common.write_report(out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
