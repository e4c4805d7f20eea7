"""Time the essential-dynamics path (metrics.ensemble_covariance and the eigenproblem behind metrics.pca) split into its three parts.

    python tools/pca_timing.py [--out profiles/pca_timing.md]      all cases, each in a child process under its own time limit
    python tools/pca_timing.py --case pca_10000_L256               one case, one JSON line

Cases: 10 000 structures of 256 residues (the headline chain length) and of 1024 (the cap).  The structures are the CA atoms of the noisy
copies of the lambda-repressor backbone of tools/timing_common.py, cut or tiled to the length.  Timed, each repetition between its own
pair of device events after warm-up: the five superposition rounds (ops.ca_fit_transforms: five s2s_ca_superpose and four
s2s_ca_aligned_mean launches), and the mean and covariance under the final transforms (s2s_ca_aligned_mean, then the prepass and the
product kernel of s2s_ca_covariance; its share alone is also given).  The host part -- the copy of the covariance and the ten largest
eigenpairs by scipy.linalg.eigh, as metrics.pca asks for them -- is timed once with the wall clock.  There is no pass/fail condition and
no other implementation to compare with: the report records what the run gives."""
import os
import sys
import time

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

CASES = {"pca_10000_L256": (10000, 256), "pca_10000_L1024": (10000, 1024)}
REPEATS = 3
CASE_TIMEOUT_S = 420


def run_case(name):
    import torch

    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    n, L = CASES[name]
    atoms, _, _ = timing_common.lambda_backbone_ensemble(n, L)
    ca = atoms[:, :, 1].contiguous()
    del atoms
    fit_ms = timing_common.time_repetitions(lambda: ops.ca_fit_transforms(ca), REPEATS, warmup=1)
    xform = ops.ca_fit_transforms(ca)
    mean = ops.ca_aligned_mean(ca, xform)
    moments_ms = timing_common.time_repetitions(lambda: ops.ca_covariance(ca, ops.ca_aligned_mean(ca, xform), xform), REPEATS, warmup=1)
    cov_ms = timing_common.time_repetitions(lambda: ops.ca_covariance(ca, mean, xform), REPEATS, warmup=1)
    cov = ops.ca_covariance(ca, mean, xform)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    variances, _ = metrics._top_components(cov.cpu().numpy(), 10)
    eigh_s = time.perf_counter() - t0
    nblk = -(-3 * L // 48)
    return {"case": name, "n": n, "L": L, "device": torch.cuda.get_device_name(0), "fit_ms": fit_ms, "moments_ms": moments_ms, "cov_ms": cov_ms,
            "eigh_s": eigh_s, "blocks": nblk * (nblk + 1) // 2, "flops": 2.0 * n * (48 * 48) * (nblk * (nblk + 1) // 2),
            "trace": float(cov.diagonal().sum()), "top_variance": float(variances[0]), "symmetric": bool(torch.equal(cov, cov.T))}


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "pca_timing.md"), CASE_TIMEOUT_S)
    if rows is None:
        return 0
    fmt = lambda ts: ", ".join(f"{t:.2f}" for t in ts)   # noqa: E731
    lines = ["# Essential dynamics: ensemble_covariance and the eigenproblem of pca", "",
             f"Device: {rows[0]['device']}.  `python tools/pca_timing.py`; every repetition of a device part between its own pair of device "
             "events, after warm-up; the host part once with the wall clock (all measured).  Inputs: the CA atoms of noisy copies "
             "(0.02 .. 1 A) of the backbone of `tests/golden/pdb/lambda.pdb` cut or tiled to the length.  No pass/fail condition and nothing to "
             "compare with: this is the record of one run.", "",
             "| case | superposition rounds (ms) | mean + covariance (ms) | covariance alone (ms) | host: copy + top-10 eigh (s) | tr C (A^2) | top variance (A^2) |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {fmt(r['fit_ms'])} | {fmt(r['moments_ms'])} | {fmt(r['cov_ms'])} | {r['eigh_s']:.2f} | {r['trace']:.2f} | "
                     f"{r['top_variance']:.2f} |")
    lines += ["", "What the fastest covariance call sustains (derived from the measured time and the counted work: 48 x 48 x R multiply-adds per "
              "upper-triangle block, one wave per block; the prepass is inside the time):", "",
              "| case | upper-triangle blocks (= waves) | float64 flop per call | float64 flop / s |", "|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['blocks']} | {r['flops']:.3e} | {r['flops'] / (min(r['cov_ms']) * 1e-3):.3e} |")
    lines.append("")
    timing_common.write_report(out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
