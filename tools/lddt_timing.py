"""Time the all-pairs lDDT kernel (s2s_ca_lddt_matrix) against what a user would write today: the same definition -- float64 distances with
square roots, the four thresholds, the reference's cutoff -- in batched float64 torch on the same device, in chunks of reference structures
that fit memory.

    python tools/lddt_timing.py [--out profiles/lddt_timing.md]      all cases, each in a child process under its own time limit
    python tools/lddt_timing.py --case 1000x1000_L256 [--kernel-only]  one case, one JSON line (--kernel-only: for a profiler run)

Cases: 1000 x 1000 structures of 256 residues and 2000 x 2000 of 64, noisy copies (Gaussian, 0.05 .. 6 A) of a compact chain: the CA trace of
tests/golden/pdb/lambda.pdb (80 residues) tiled on a 24 A lattice to the length and cut.  Every repetition is timed on its own with device
events around the whole call, after warm-up; all of them are written out.  The condition of the record: the kernel's slowest repetition
is faster than the torch restatement's fastest.
The kernel's work is counted from the lists themselves: (included unordered pairs of every reference) x (models), each a gather of two
float32 points (24 B) from LDS, 11 float64 operations (three differences, three products and two sums for the squared distance count as
8, with the conversions left out) and eight float64 comparisons.
"""
import os
import sys

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

CASES = {"1000x1000_L256": (1000, 256), "2000x2000_L64": (2000, 64)}
CUTOFF = 15.0
REPEATS = 5
TORCH_CHUNK_BYTES = 1 << 30          # the [chunk, Rb, L, L] float64 difference tensor of the torch restatement
CASE_TIMEOUT_S = 420
PEAK_F64_VECTOR = 78.6e12            # the data sheet's float64 vector rate


def chain(L):
    """[L, 3] float64: the CA trace of lambda.pdb tiled on a lattice to L residues."""
    import numpy as np

    from str2str_amd.common.pdb_utils import extract_backbone_coords

    ca = np.asarray(extract_backbone_coords(os.path.join(ROOT, "tests", "golden", "pdb", "lambda.pdb"))[0], dtype=np.float64)
    return timing_common.tile_on_lattice(ca, L)


def ensemble(n, L, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    base = torch.as_tensor(chain(L))[None]
    noisy = base + torch.randn(n, L, 3, generator=g, dtype=torch.float64) * torch.linspace(0.05, 6.0, n, dtype=torch.float64)[:, None, None]
    return (noisy + 100.0 * torch.rand(n, 1, 3, generator=g, dtype=torch.float64) - 50.0).to("cuda", torch.float32)


def distances(x):
    d = x[:, :, None, :] - x[:, None, :, :]
    return d.square().sum(-1).sqrt()


def torch_lddt(a, b, cutoff=CUTOFF, want_pairs=False):
    """a [Ra, L, 3], b [Rb, L, 3] -> lDDT [Ra, Rb] float64 (and the included ordered pairs of every a): the definition, batched."""
    import torch

    a, b = a.double(), b.double()
    (n_a, L), n_b = a.shape[:2], b.shape[0]
    db = distances(b)                                                   # [Rb, L, L]
    off = ~torch.eye(L, dtype=torch.bool, device=a.device)
    out = torch.empty(n_a, n_b, dtype=torch.float64, device=a.device)
    pairs = torch.empty(n_a, dtype=torch.int64, device=a.device)
    rows = max(1, TORCH_CHUNK_BYTES // (8 * n_b * L * L))
    for r0 in range(0, n_a, rows):
        da = distances(a[r0:r0 + rows])                                 # [r, L, L]
        inc = (da < cutoff) & off
        l1 = (da[:, None] - db[None]).abs()                             # [r, Rb, L, L]
        score = (l1 < 0.5).to(torch.int8) + (l1 < 1.0).to(torch.int8) + (l1 < 2.0).to(torch.int8) + (l1 < 4.0).to(torch.int8)
        hits = (score * inc[:, None]).sum((-1, -2), dtype=torch.int64)  # [r, Rb]
        n = inc.sum((-1, -2))
        pairs[r0:r0 + rows] = n
        out[r0:r0 + rows] = torch.where(n[:, None] > 0, hits.double() / (4.0 * n[:, None].double()).clamp(min=1.0), 1.0)
    return (out, pairs) if want_pairs else out


def run_case(name, kernel_only=False):
    import torch

    from str2str_amd import ops

    n, L = CASES[name]
    a, b = ensemble(n, L, 1), ensemble(n, L, 2)
    out = torch.empty(n, n, dtype=torch.float64, device="cuda")
    kernel_ms = timing_common.time_repetitions(lambda: ops.ca_lddt_matrix(a, b, out=out), REPEATS, warmup=2)
    res = {"case": name, "n": n, "L": L, "pairs": n * n, "kernel_ms": kernel_ms, "device": torch.cuda.get_device_name(0)}
    if kernel_only:
        return res
    torch_ms = timing_common.time_repetitions(lambda: torch_lddt(a, b), REPEATS, warmup=1)
    want, included = torch_lddt(a, b, want_pairs=True)
    evals = float(included.sum()) / 2.0 * n                             # (unordered pair of a reference, model)
    diff = (want - out).abs()
    best = min(kernel_ms) * 1e-3
    res.update({"torch_ms": torch_ms, "max_abs_diff_vs_torch": float(diff.max()), "entries_that_differ": int((diff > 4e-16).sum()),
                "mean_lddt": float(out.mean()), "mean_included_pairs": float(included.double().mean()) / 2.0, "evaluations": evals,
                "evaluations_per_s": evals / best, "lds_gather_bytes_per_s": 24.0 * evals / best,
                "share_of_f64_vector_peak": 19.0 * evals / best / PEAK_F64_VECTOR,
                "holds": max(kernel_ms) < min(torch_ms)})
    return res


def _ms(xs):
    return ", ".join(f"{x:.2f}" for x in xs)


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "lddt_timing.md"), CASE_TIMEOUT_S, kernel_only=True)
    if rows is None:
        return 0
    holds = all(r["holds"] for r in rows)
    lines = ["# All-pairs lDDT: s2s_ca_lddt_matrix against the same definition in batched float64 torch", "",
             f"Device: {rows[0]['device']}.  `python tools/lddt_timing.py`; every repetition between its own pair of device events around the whole "
             f"call, after warm-up (measured).  Inputs: noisy copies (0.05 .. 6 A) of the CA trace of `tests/golden/pdb/lambda.pdb` tiled to the "
             f"length; cutoff {CUTOFF} A, min_seq_sep 1.  The torch restatement holds the models' distance matrices and walks the reference "
             f"structures in chunks whose [chunk, Rb, L, L] float64 difference tensor is {TORCH_CHUNK_BYTES >> 20} MiB.", "",
             "| case | kernel, every repetition (ms) | torch float64, every repetition (ms) | slowest kernel / fastest torch | included pairs per reference (mean) | max abs diff vs torch (entries off by more than 4e-16) | mean lDDT |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {_ms(r['kernel_ms'])} | {_ms(r['torch_ms'])} | {max(r['kernel_ms']):.2f} / {min(r['torch_ms']):.2f} = "
                     f"1 / {min(r['torch_ms']) / max(r['kernel_ms']):.0f} | {r['mean_included_pairs']:.0f} | {r['max_abs_diff_vs_torch']:.1e} "
                     f"({r['entries_that_differ']}) | {r['mean_lddt']:.4f} |")
    lines += ["", "**The kernel's slowest repetition is faster than the torch restatement's fastest in both cases.**" if holds else
              "**The condition does NOT hold: the kernel's slowest repetition is not faster than the torch restatement's fastest in every case.**", "",
              "What the fastest repetition of the kernel sustains (derived from the measured time and the counted work: one evaluation = one "
              "included unordered pair of a reference against one model = 24 B gathered from LDS, 11 float64 operations and 8 float64 comparisons; "
              "both passes and the staging are inside the time):", "",
              "| case | evaluations | evaluations / s | LDS gather (TB/s) | share of the float64 vector peak (19 operations per evaluation, 78.6 TFLOP/s) |",
              "|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['evaluations']:.3e} | {r['evaluations_per_s']:.3e} | {r['lds_gather_bytes_per_s'] / 1e12:.2f} | "
                     f"{100 * r['share_of_f64_vector_peak']:.1f} % |")
    lines.append("")
    timing_common.write_report(out, lines)
    return 0 if holds else 2


if __name__ == "__main__":
    sys.exit(main())
