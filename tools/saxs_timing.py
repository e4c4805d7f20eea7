"""Time the solution-scattering kernel (s2s_ca_scattering) and count its work.

    python tools/saxs_timing.py [--out profiles/saxs_timing.md]      all cases, each in a child process under its own time limit
    python tools/saxs_timing.py --case saxs_10000_L256_Q64           one case, one JSON line

Cases: 10 000 structures of 256 residues at 64 and at 512 q-values (the sizes of a coarse and of a measured grid), and one structure of
1024 residues (the cap) at 512 q-values, where the grid is a single structure's q-tiles.  The structures are the CA atoms of the noisy copies of
the lambda-repressor backbone of tools/timing_common.py, cut or tiled to the length; q is uniform on 0 .. 0.5 per Angstrom, the form
factors are the default.  Every repetition is timed on its own with device events around the whole call (the upload of q, the types and
the table included), after warm-up; all of them are written out.  There is no pass/fail condition and no other implementation to compare
with: the report records what the run gives.
The kernel's work is counted from its definition: a sinc evaluation is one (pair, q) term -- one product, one double sine, one division,
one product with f_i f_j and one addition --, R L (L - 1) / 2 Q of them per call."""
import os
import sys

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

CASES = {"saxs_10000_L256_Q64": (10000, 256, 64), "saxs_10000_L256_Q512": (10000, 256, 512), "saxs_1_L1024_Q512": (1, 1024, 512)}
REPEATS = 5
CASE_TIMEOUT_S = 300


def run_case(name):
    import numpy as np
    import torch

    from str2str_amd import ops

    n, L, Q = CASES[name]
    atoms, _, _ = timing_common.lambda_backbone_ensemble(n, L)
    ca = atoms[:, :, 1].contiguous()
    q = np.linspace(0.0, 0.5, Q)
    ms = timing_common.time_repetitions(lambda: ops.ca_scattering(ca, q), REPEATS, warmup=2)
    intensity, inv_r_mean = ops.ca_scattering(ca, q)
    return {"case": name, "n": n, "L": L, "Q": Q, "device": torch.cuda.get_device_name(0), "call_ms": ms,
            "sinc_evaluations": float(n) * (L * (L - 1) // 2) * Q, "forward_over_L2": float(intensity[:, 0].mean()) / float(L * L),
            "last_over_first": float((intensity[:, -1] / intensity[:, 0]).mean()), "mean_rh_A": float((1.0 / inv_r_mean).mean())}


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "saxs_timing.md"), CASE_TIMEOUT_S)
    if rows is None:
        return 0
    lines = ["# Solution scattering: s2s_ca_scattering", "",
             f"Device: {rows[0]['device']}.  `python tools/saxs_timing.py`; every repetition between its own pair of device events around the "
             "whole call, after warm-up (measured).  Inputs: the CA atoms of noisy copies (0.02 .. 1 A) of the backbone of "
             "`tests/golden/pdb/lambda.pdb` cut or tiled to the length, q uniform on 0 .. 0.5 / A, default form factors.  No pass/fail "
             "condition and nothing to compare with: this is the record of one run.", "",
             "| case | every repetition (ms) | structures / s | I(0) / L^2 | I(0.5) / I(0) | mean Rh (A) |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {', '.join(f'{t:.2f}' for t in r['call_ms'])} | {r['n'] / (min(r['call_ms']) * 1e-3):.3e} | {r['forward_over_L2']:.6f} | "
                     f"{r['last_over_first']:.3e} | {r['mean_rh_A']:.2f} |")
    lines += ["", "What the fastest repetition sustains (derived from the measured time and the counted work: a sinc evaluation is one (pair, q) "
              "term, a product, a double sine, a division, a product and an addition; staging and the sums are inside the time):", "",
              "| case | pairs per structure | sinc evaluations per call | sinc evaluations / s |", "|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['L'] * (r['L'] - 1) // 2} | {r['sinc_evaluations']:.3e} | {r['sinc_evaluations'] / (min(r['call_ms']) * 1e-3):.3e} |")
    lines.append("")
    timing_common.write_report(out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
