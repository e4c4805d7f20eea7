"""Time the solvent-accessibility kernel (s2s_backbone_sasa) and count its work.

    python tools/sasa_timing.py [--out profiles/sasa_timing.md]      all cases, each in a child process under its own time limit
    python tools/sasa_timing.py --case sasa_10000_L256_P96            one case, one JSON line

Cases: 10 000 structures of 256 residues at 96 and at 960 points per atom, and short chains as the fast-folder workload has them (12 000
structures of 35 residues, 96 points).  The structures are the noisy copies of the lambda-repressor backbone of tools/timing_common.py, cut
or tiled to the length; radii and probe are the metrics layer's defaults.  Every repetition is timed on its own with device events around
the whole call (the upload of the sphere, the radii and the existence flags included), after warm-up; all of them are written out.  There
is no pass/fail condition and no other implementation to compare with: the report records what the run gives, and the figure to set it
against is the float64 vector rate of the device.
The kernel's work is counted from its outputs' definition, not from what it skips: a point test is one (point, other atom) pair, 3
differences, 3 products, 2 sums and a comparison in float64.  ``tests_brute`` is what the definition asks for, P x A x (A - 1) per
structure; ``tests_near`` counts only the pairs whose expanded spheres intersect, |c_a - c_b| < R_a + R_b, the tests the prefilter leaves
when no sweep ends early (an upper bound of what the kernel does: it stops an atom's sweep once all its points are buried, and drops
points as they are buried only from the bookkeeping, not from the arithmetic of their lane)."""
import os
import sys

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

CASES = {"sasa_10000_L256_P96": (10000, 256, 96), "sasa_10000_L256_P960": (10000, 256, 960), "sasa_12000_L35_P96": (12000, 35, 96)}
REPEATS = 5
CASE_TIMEOUT_S = 300
PEAK_F64_VECTOR = 78.6e12            # the data sheet's float64 vector rate
OPS_PER_TEST = 9


def near_pairs(x, exists, radii, probe, sample=8):
    """The mean number of ordered atom pairs with intersecting expanded spheres over ``sample`` structures spread through the ensemble."""
    import torch

    idx = torch.linspace(0, x.shape[0] - 1, sample).long().to(x.device)
    c = x[idx].double().reshape(sample, -1, 3)
    ex = torch.as_tensor(exists.reshape(-1) != 0, device=x.device)
    R = torch.as_tensor(radii.reshape(-1) + probe, device=x.device)
    d = (c[:, :, None] - c[:, None]).norm(dim=-1)
    hit = (d < R[:, None] + R[None, :]) & ex[:, None] & ex[None, :]
    return float(hit.sum()) / sample - float(ex.sum())


def run_case(name):
    import numpy as np
    import torch

    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    n, L, P = CASES[name]
    x, aatype, _ = timing_common.lambda_backbone_ensemble(n, L)
    exists = np.ones((L, 5), dtype=np.uint8)
    exists[aatype == metrics.GLY, 4] = 0
    radii = np.tile(np.asarray(metrics.SASA_RADII), (L, 1))
    ms = timing_common.time_repetitions(lambda: ops.backbone_sasa(x, exists, radii, 1.4, P), REPEATS, warmup=2)
    counts, _, total = ops.backbone_sasa(x, exists, radii, 1.4, P)
    A = int(exists.sum())
    best = min(ms) * 1e-3
    near = near_pairs(x, exists, radii, 1.4)
    return {"case": name, "n": n, "L": L, "P": P, "device": torch.cuda.get_device_name(0), "kernel_ms": ms, "atoms": A,
            "near_pairs_per_structure": near, "tests_brute": float(n) * P * A * (A - 1), "tests_near": float(n) * P * near,
            "structures_per_s": n / best, "mean_total_A2": float(total.mean()), "accessible_share_of_points": float(counts.sum()) / (float(n) * P * A)}


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "sasa_timing.md"), CASE_TIMEOUT_S)
    if rows is None:
        return 0
    lines = ["# Solvent accessibility: s2s_backbone_sasa", "",
             f"Device: {rows[0]['device']}.  `python tools/sasa_timing.py`; every repetition between its own pair of device events around the "
             "whole call, after warm-up (measured).  Inputs: noisy copies (0.02 .. 1 A) of the backbone of `tests/golden/pdb/lambda.pdb` cut or "
             "tiled to the length, Bondi radii, probe 1.4 A.  No pass/fail condition and nothing to compare with: this is the record of one run.", "",
             "| case | every repetition (ms) | structures / s | mean total (A^2) | accessible share of the points |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {', '.join(f'{t:.2f}' for t in r['kernel_ms'])} | {r['structures_per_s']:.3e} | {r['mean_total_A2']:.1f} | "
                     f"{r['accessible_share_of_points']:.3f} |")
    lines += ["", "What the fastest repetition sustains (derived from the measured time and the counted work: a point test is one point against one "
              f"other atom, {OPS_PER_TEST} float64 operations; `brute` counts every pair the definition names, `near` only the pairs whose expanded "
              "spheres intersect, an upper bound of what the kernel evaluates; staging and the sums are inside the time):", "",
              "| case | atoms | near atoms per atom | point tests, brute | brute tests / s | point tests, near | near tests / s | share of the float64 "
              "vector peak (near tests, 78.6 TFLOP/s) |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        best = min(r["kernel_ms"]) * 1e-3
        lines.append(f"| {r['case']} | {r['atoms']} | {r['near_pairs_per_structure'] / r['atoms']:.1f} | {r['tests_brute']:.3e} | {r['tests_brute'] / best:.3e} | "
                     f"{r['tests_near']:.3e} | {r['tests_near'] / best:.3e} | {100 * OPS_PER_TEST * r['tests_near'] / best / PEAK_F64_VECTOR:.1f} % |")
    lines.append("")
    timing_common.write_report(out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
