"""Time the secondary-structure kernel (s2s_secondary_structure) at three chain lengths.

    python tools/ss_timing.py [--out profiles/ss_timing.md]     all cases, each in a child process under its own time limit
    python tools/ss_timing.py --case 10000x256                    one case, one JSON line (for a profiler run)

Cases: 20 000 structures of 64 residues, 10 000 of 256 and 4 000 of 512: noisy copies (Gaussian, 0.02 .. 1 A on every atom) of the backbone
of tests/golden/pdb/lambda.pdb (80 residues, five helices) cut or tiled on a 24 A lattice to the length, numbered with a gap between the
copies.  Every repetition is timed on its own with device events around the whole call (one launch: staging, hydrogens and torsions, the
hydrogen-bond sweep, patterns, states), after warm-up; all of them are written out.  The share of (acceptor, donor) residue pairs that
pass the 9 A CA prefilter -- the pairs whose energy is evaluated -- is counted in torch from the CA atoms of the first 16 structures."""
import os
import sys

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

CASES = {"20000x64": (20000, 64), "10000x256": (10000, 256), "4000x512": (4000, 512)}
REPEATS = 5
CASE_TIMEOUT_S = 300


def survivors(atoms):
    """The share of ordered residue pairs (i, j != i) of atoms [n, L, 5, 3] with |CA_i - CA_j| < 9 A."""
    import torch

    ca = atoms[:, :, 1].double()
    d = (ca[:, :, None] - ca[:, None, :]).square().sum(-1).sqrt()
    L = d.shape[1]
    off = ~torch.eye(L, dtype=torch.bool, device=d.device)
    return float(((d < 9.0) & off).sum()) / float(off.sum() * d.shape[0])


def run_case(name):
    import numpy as np
    import torch

    from str2str_amd import ops

    n, L = CASES[name]
    atoms, aatype, per = timing_common.lambda_backbone_ensemble(n, L)
    residue_index = np.arange(L) + 10 * (np.arange(L) // per)          # a numbering gap between the copies
    ms = timing_common.time_repetitions(lambda: ops.secondary_structure(atoms, aatype, residue_index), REPEATS, warmup=2)
    ss, n_hbonds, _, _, _ = ops.secondary_structure(atoms, aatype, residue_index)
    helix = float(((ss == ord("H")) | (ss == ord("G")) | (ss == ord("I"))).double().mean())
    return {"case": name, "n": n, "L": L, "kernel_ms": ms, "structures_per_s": n / (min(ms) * 1e-3),
            "residue_pairs_per_s": n * (L * (L - 1)) / (min(ms) * 1e-3), "pairs_passing_prefilter": survivors(atoms[:16]),
            "mean_hbonds": float(n_hbonds.double().mean()), "helix_fraction": helix, "device": torch.cuda.get_device_name(0)}


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "ss_timing.md"), CASE_TIMEOUT_S)
    if rows is None:
        return 0
    lines = ["# Secondary structure and torsions: s2s_secondary_structure", "",
             f"Device: {rows[0]['device']}.  `python tools/ss_timing.py`; every repetition between its own pair of device events around the "
             "whole call (one launch: staging, hydrogens and torsions, hydrogen-bond sweep, patterns, states), after warm-up (measured).  "
             "Structures: noisy copies (0.02 .. 1 A per atom) of the backbone of `tests/golden/pdb/lambda.pdb` cut or tiled to the length.", "",
             "| case (structures x residues) | every repetition (ms) | structures / s (fastest) | ordered residue pairs / s | pairs passing the 9 A prefilter | hydrogen bonds per structure (mean) | helix fraction |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {', '.join(f'{x:.2f}' for x in r['kernel_ms'])} | {r['structures_per_s']:.3e} | {r['residue_pairs_per_s']:.3e} | "
                     f"{100 * r['pairs_passing_prefilter']:.1f} % | {r['mean_hbonds']:.1f} | {r['helix_fraction']:.3f} |")
    lines.append("")
    timing_common.write_report(out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
