"""What the ensemble timing scripts (rmsd, tm, lddt, violations, ss) share: the two device-event timers, the command line that runs one
case here or every case in a child process of its own, and the ensemble of noisy lambda-repressor backbones."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE = 24.0                       # A between the tiled copies of the chain (its radius of gyration is 11.4 A)


def time_repetitions(fn, repeats=5, warmup=2):
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


def time_window(fn, min_window_s=0.5, warmup=3):
    """-> (mean time of a repetition (ms), repetitions): as many as fill a window of ``min_window_s``, each between its own device events."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    while total < min_window_s * 1e3 and reps < 5000:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
        reps += 1
    return total / reps, reps


def tile_on_lattice(chain, L):
    """chain [per, ...] float64 -> [L, ...]: copies of it on a lattice of LATTICE A, cut to L residues."""
    import numpy as np

    copies = -(-L // len(chain))
    cells = [(i, j, k) for k in range(copies) for j in range(2) for i in range(2)][:copies]
    return np.concatenate([chain + LATTICE * np.asarray(c, dtype=np.float64) for c in cells])[:L]


def lambda_backbone_ensemble(n, L, seed=1, scale=1.0):
    """-> (atoms [n, L, 5, 3] float32 on the device, aatype [L], the residues of one copy): noisy copies (Gaussian, 0.02 .. 1 A on every
    atom) of the backbone of tests/golden/pdb/lambda.pdb (80 residues) cut or tiled to L residues, times ``scale``."""
    import numpy as np
    import torch

    from str2str_amd.common.pdb_utils import extract_backbone_atoms

    atoms, aatype, _ = extract_backbone_atoms(os.path.join(ROOT, "tests", "golden", "pdb", "lambda.pdb"))
    per = atoms.shape[1]
    base = tile_on_lattice(atoms[0].astype(np.float64), L)
    g = torch.Generator().manual_seed(seed)
    x = torch.as_tensor(base)[None] + torch.randn(n, L, 5, 3, generator=g, dtype=torch.float64) * torch.linspace(0.02, 1.0, n, dtype=torch.float64)[:, None, None, None]
    return (x * scale).to("cuda", torch.float32), np.tile(aatype, -(-L // per))[:L], per


def collect(script, cases, run_case, default_out, case_timeout_s, kernel_only=False):
    """The command line of a timing script.  ``--case NAME`` runs that case in this process, prints its one JSON line and returns
    (None, None).  Without it every case runs in a child process of its own under ``case_timeout_s``; nothing more is started after a case
    that fails or runs out of time (the process then ends with that case's code); -> (the cases' results, the ``--out`` path).
    ``kernel_only``: the script takes ``--kernel-only`` and passes it to ``run_case``."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(cases))
    if kernel_only:
        ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=default_out)
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(args.case, args.kernel_only) if kernel_only else run_case(args.case)), flush=True)
        return None, None
    rows = []
    for name in cases:
        p = subprocess.run([sys.executable, os.path.abspath(script), "--case", name], capture_output=True, text=True, timeout=case_timeout_s)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode or 1)
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(rows[-1], flush=True)
    return rows, args.out


def write_report(path, lines):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines))
