"""Time the secondary-structure kernel (s2s_secondary_structure) at three chain lengths.

    python tools/ss_timing.py [--out profiles/ss_timing.md]     all cases, each in a child process under its own time limit
    python tools/ss_timing.py --case 10000x256                    one case, one JSON line (for a profiler run)

Cases: 20 000 structures of 64 residues, 10 000 of 256 and 4 000 of 512: noisy copies (Gaussian, 0.02 .. 1 A on every atom) of the backbone
of tests/golden/pdb/lambda.pdb (80 residues, five helices) cut or tiled on a 24 A lattice to the length, numbered with a gap between the
copies.  Every repetition is timed on its own with device events around the whole call (one launch: staging, hydrogens and torsions, the
hydrogen-bond sweep, patterns, states), after warm-up; all of them are written out.  The share of (acceptor, donor) residue pairs that
pass the 9 A CA prefilter -- the pairs whose energy is evaluated -- is counted in torch from the CA atoms of the first 16 structures."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"20000x64": (20000, 64), "10000x256": (10000, 256), "4000x512": (4000, 512)}
REPEATS = 5
CASE_TIMEOUT_S = 300
LATTICE = 24.0                       # A between the tiled copies of the chain (its radius of gyration is 11.4 A)


def ensemble(n, L, seed=1):
    """-> (atoms [n, L, 5, 3] float32 on the device, aatype [L], residue_index [L])."""
    import numpy as np
    import torch

    from str2str_amd.common.pdb_utils import extract_backbone_atoms

    atoms, aatype, _ = extract_backbone_atoms(os.path.join(ROOT, "tests", "golden", "pdb", "lambda.pdb"))
    per = atoms.shape[1]
    copies = -(-L // per)
    cells = [(i, j, k) for k in range(copies) for j in range(2) for i in range(2)][:copies]
    base = np.concatenate([atoms[0].astype(np.float64) + LATTICE * np.asarray(c, dtype=np.float64) for c in cells])[:L]
    g = torch.Generator().manual_seed(seed)
    x = torch.as_tensor(base)[None] + torch.randn(n, L, 5, 3, generator=g, dtype=torch.float64) * torch.linspace(0.02, 1.0, n, dtype=torch.float64)[:, None, None, None]
    residue_index = np.arange(L) + 10 * (np.arange(L) // per)          # a numbering gap between the copies
    return x.to("cuda", torch.float32), np.tile(aatype, copies)[:L], residue_index


def survivors(atoms):
    """The share of ordered residue pairs (i, j != i) of atoms [n, L, 5, 3] with |CA_i - CA_j| < 9 A."""
    import torch

    ca = atoms[:, :, 1].double()
    d = (ca[:, :, None] - ca[:, None, :]).square().sum(-1).sqrt()
    L = d.shape[1]
    off = ~torch.eye(L, dtype=torch.bool, device=d.device)
    return float(((d < 9.0) & off).sum()) / float(off.sum() * d.shape[0])


def timed(fn, repeats=REPEATS, warmup=2):
    """-> the time of every repetition (ms), each between its own pair of device events."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def run_case(name):
    import torch

    from str2str_amd import ops

    n, L = CASES[name]
    atoms, aatype, residue_index = ensemble(n, L)
    ms = timed(lambda: ops.secondary_structure(atoms, aatype, residue_index))
    ss, n_hbonds, _, _, _ = ops.secondary_structure(atoms, aatype, residue_index)
    helix = float(((ss == ord("H")) | (ss == ord("G")) | (ss == ord("I"))).double().mean())
    return {"case": name, "n": n, "L": L, "kernel_ms": ms, "structures_per_s": n / (min(ms) * 1e-3),
            "residue_pairs_per_s": n * (L * (L - 1)) / (min(ms) * 1e-3), "pairs_passing_prefilter": survivors(atoms[:16]),
            "mean_hbonds": float(n_hbonds.double().mean()), "helix_fraction": helix, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ss_timing.md"))
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(args.case)), flush=True)
        return 0
    rows = []
    for name in CASES:      # one child per case, each under its own time limit; nothing more is started after a failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], capture_output=True, text=True, timeout=CASE_TIMEOUT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            return p.returncode or 1
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(rows[-1], flush=True)
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
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
