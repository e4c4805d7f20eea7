"""Time the backbone-violation kernel (s2s_backbone_violations) and show what its residue prefilter is worth.

    python tools/violations_timing.py [--out profiles/violations_timing.md]     all cases, each in a child process under its own time limit
    python tools/violations_timing.py --case 10000x256_chain                       one case, one JSON line (for a profiler run)

Cases: 10 000 structures of 256 residues and 1 000 of 1 024, each as ``chain`` -- noisy copies (Gaussian, 0.02 .. 1 A on every atom) of
the backbone of tests/golden/pdb/lambda.pdb (80 residues) tiled on a 24 A lattice to the length, where a residue has a handful of
neighbours within the prefilter's reach -- and as ``globule``: the same structures shrunk to a tenth, in which most residue pairs pass the
prefilter and are expanded into their 25 atom pairs, the work the kernel would do everywhere without it.  Every repetition is timed on its
own with device events around the whole call, after warm-up; all of them are written out.  The share of residue pairs that pass the
prefilter is counted in torch from the CA atoms of the first 16 structures."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"10000x256": (10000, 256), "1000x1024": (1000, 1024)}
CASES = {f"{size}_{kind}": (size, kind) for size in SIZES for kind in ("chain", "globule")}
REPEATS = 5
CASE_TIMEOUT_S = 300
LATTICE = 24.0                       # A between the tiled copies of the chain (its radius of gyration is 11.4 A)
SHRINK = 0.1


def ensemble(n, L, kind, seed=1):
    """-> (atoms [n, L, 5, 3] float32 on the device, aatype [L], residue_index [L])."""
    import numpy as np
    import torch

    from str2str_amd.common.pdb_utils import extract_backbone_atoms

    atoms, aatype, _ = extract_backbone_atoms(os.path.join(ROOT, "tests", "golden", "pdb", "lambda.pdb"))
    copies = -(-L // atoms.shape[1])
    cells = [(i, j, k) for k in range(copies) for j in range(2) for i in range(2)][:copies]
    base = np.concatenate([atoms[0].astype(np.float64) + LATTICE * np.asarray(c, dtype=np.float64) for c in cells])[:L]
    g = torch.Generator().manual_seed(seed)
    x = torch.as_tensor(base)[None] + torch.randn(n, L, 5, 3, generator=g, dtype=torch.float64) * torch.linspace(0.02, 1.0, n, dtype=torch.float64)[:, None, None, None]
    if kind == "globule":
        x = x * SHRINK
    return x.to("cuda", torch.float32), np.tile(aatype, copies)[:L], np.arange(L)


def survivors(atoms, exists, clash_tolerance=1.5):
    """The share of residue pairs i < j of atoms [n, L, 5, 3] that pass d(CA_i, CA_j) < rho_i + rho_j + (3.4 - clash_tolerance)."""
    import torch

    x = atoms.double()
    rho = ((x - x[:, :, 1:2]).square().sum(-1).sqrt() * torch.as_tensor(exists, device=x.device)).amax(-1)
    d = (x[:, :, None, 1] - x[:, None, :, 1]).square().sum(-1).sqrt()
    upper = torch.triu(torch.ones(d.shape[1:], dtype=torch.bool, device=x.device), 1)
    return float(((d < rho[:, :, None] + rho[:, None, :] + (3.4 - clash_tolerance)) & upper).sum()) / float(upper.sum() * x.shape[0])


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
    import numpy as np
    import torch

    from str2str_amd import ops

    size, kind = CASES[name]
    n, L = SIZES[size]
    atoms, aatype, residue_index = ensemble(n, L, kind)
    exists = np.ones((L, 5), dtype=np.uint8)
    exists[aatype == 7, 4] = 0
    ms = timed(lambda: ops.backbone_violations(atoms, exists, aatype, residue_index))
    out = ops.backbone_violations(atoms, exists, aatype, residue_index)
    return {"case": name, "n": n, "L": L, "kind": kind, "kernel_ms": ms, "structures_per_s": n / (min(ms) * 1e-3),
            "residue_pairs_per_s": n * (L * (L - 1) / 2) / (min(ms) * 1e-3), "pairs_passing_prefilter": survivors(atoms[:16], exists),
            "mean_clashing_atom_pairs": float(out[5].double().mean()), "mean_violations_per_residue": float(out[1][:, 2].mean()),
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "violations_timing.md"))
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
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
