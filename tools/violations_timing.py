"""Time the backbone-violation kernel (s2s_backbone_violations) and show what its residue prefilter is worth.

    python tools/violations_timing.py [--out profiles/violations_timing.md]     all cases, each in a child process under its own time limit
    python tools/violations_timing.py --case 10000x256_chain                       one case, one JSON line (for a profiler run)

Cases: 10 000 structures of 256 residues and 1 000 of 1 024, each as ``chain`` -- noisy copies (Gaussian, 0.02 .. 1 A on every atom) of
the backbone of tests/golden/pdb/lambda.pdb (80 residues) tiled on a 24 A lattice to the length, where a residue has a handful of
neighbours within the prefilter's reach -- and as ``globule``: the same structures shrunk to a tenth, in which most residue pairs pass the
prefilter and are expanded into their 25 atom pairs, the work the kernel would do everywhere without it.  Every repetition is timed on its
own with device events around the whole call, after warm-up; all of them are written out.  The share of residue pairs that pass the
prefilter is counted in torch from the CA atoms of the first 16 structures."""
import os
import sys

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

SIZES = {"10000x256": (10000, 256), "1000x1024": (1000, 1024)}
CASES = {f"{size}_{kind}": (size, kind) for size in SIZES for kind in ("chain", "globule")}
REPEATS = 5
CASE_TIMEOUT_S = 300
SHRINK = 0.1


def survivors(atoms, exists, clash_tolerance=1.5):
    """The share of residue pairs i < j of atoms [n, L, 5, 3] that pass d(CA_i, CA_j) < rho_i + rho_j + (3.4 - clash_tolerance)."""
    import torch

    x = atoms.double()
    rho = ((x - x[:, :, 1:2]).square().sum(-1).sqrt() * torch.as_tensor(exists, device=x.device)).amax(-1)
    d = (x[:, :, None, 1] - x[:, None, :, 1]).square().sum(-1).sqrt()
    upper = torch.triu(torch.ones(d.shape[1:], dtype=torch.bool, device=x.device), 1)
    return float(((d < rho[:, :, None] + rho[:, None, :] + (3.4 - clash_tolerance)) & upper).sum()) / float(upper.sum() * x.shape[0])


def run_case(name):
    import numpy as np
    import torch

    from str2str_amd import ops

    size, kind = CASES[name]
    n, L = SIZES[size]
    atoms, aatype, _ = timing_common.lambda_backbone_ensemble(n, L, scale=SHRINK if kind == "globule" else 1.0)
    residue_index = np.arange(L)
    exists = np.ones((L, 5), dtype=np.uint8)
    exists[aatype == 7, 4] = 0
    ms = timing_common.time_repetitions(lambda: ops.backbone_violations(atoms, exists, aatype, residue_index), REPEATS, warmup=2)
    out = ops.backbone_violations(atoms, exists, aatype, residue_index)
    return {"case": name, "n": n, "L": L, "kind": kind, "kernel_ms": ms, "structures_per_s": n / (min(ms) * 1e-3),
            "residue_pairs_per_s": n * (L * (L - 1) / 2) / (min(ms) * 1e-3), "pairs_passing_prefilter": survivors(atoms[:16], exists),
            "mean_clashing_atom_pairs": float(out[5].double().mean()), "mean_violations_per_residue": float(out[1][:, 2].mean()),
            "device": torch.cuda.get_device_name(0)}


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "violations_timing.md"), CASE_TIMEOUT_S)
    if rows is None:
        return 0
    lines = ["# Backbone violations: s2s_backbone_violations, with and without the prefilter's effect", "",
             f"Device: {rows[0]['device']}.  `python tools/violations_timing.py`; every repetition between its own pair of device events around the "
             "whole call (one launch: staging, connection terms, prefilter sweep, atom-pair expansion, outputs), after warm-up (measured).  `chain`: "
             "noisy copies (0.02 .. 1 A per atom) of the backbone of `tests/golden/pdb/lambda.pdb` tiled to the length; `globule`: the same "
             f"shrunk to {SHRINK:g} of their size, so that most residue pairs pass the prefilter and are expanded into their 25 atom pairs.", "",
             "| case | every repetition (ms) | structures / s (fastest) | residue pairs / s | residue pairs passing the prefilter | clashing atom pairs per structure (mean) | violations_per_residue (mean) |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {', '.join(f'{x:.2f}' for x in r['kernel_ms'])} | {r['structures_per_s']:.3e} | {r['residue_pairs_per_s']:.3e} | "
                     f"{100 * r['pairs_passing_prefilter']:.1f} % | {r['mean_clashing_atom_pairs']:.1f} | {r['mean_violations_per_residue']:.3f} |")
    by = {r["case"]: r for r in rows}
    lines.append("")
    for size in SIZES:
        c, g = by[f"{size}_chain"], by[f"{size}_globule"]
        lines.append(f"- {size}: the chain, where the prefilter drops {100 * (1 - c['pairs_passing_prefilter']):.1f} % of the residue pairs, runs "
                     f"{min(g['kernel_ms']) / min(c['kernel_ms']):.1f} x faster than the globule, where it drops "
                     f"{100 * (1 - g['pairs_passing_prefilter']):.1f} %.")
    lines.append("")
    timing_common.write_report(out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
