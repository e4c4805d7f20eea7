"""Time the all-pairs minimum-RMSD kernel (s2s_ca_rmsd_matrix) against what a user would write today: the same pairs through a
batched float64 ``torch.linalg.svd`` on the same device.

    python tools/rmsd_timing.py [--out profiles/ensemble_rmsd_timing.md]      all cases, each in a child process under its own time limit
    python tools/rmsd_timing.py --case self_1000_L256                         one case, one JSON line

Cases: self matrix at R = 1000 with L = 35 and L = 256; cross matrix 1000 x 10000 at L = 256.  Times are device events around the
whole call (prepass + pair kernel), after warm-up, over enough repetitions for a window of >= 0.5 s.  The SVD baseline is timed on the
first rows of the case, BASELINE_PAIRS pairs, and scaled to all pairs (stated in the output).
"Share of the float64 matrix peak" = 2 * 9 * L flop per computed pair (the cross-covariance product only) over the kernel's time,
against the 78.6 TFLOP/s float64 matrix rate of the MI355X data sheet.
"""
import os
import sys

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

CASES = {"self_1000_L35": (1000, None, 35), "self_1000_L256": (1000, None, 256), "cross_1000x10000_L256": (1000, 10000, 256)}
PEAK_F64_MATRIX = 78.6e12
BASELINE_PAIRS = 1 << 17
CASE_TIMEOUT_S = 240


def chains(n, L, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    step = torch.randn(n, L, 3, generator=g)
    step = 3.8 * step / step.norm(dim=-1, keepdim=True)
    return (step.cumsum(1) + 100.0 * torch.rand(n, 1, 3, generator=g) - 50.0).to("cuda", torch.float32)


def svd_rmsd(a, b):
    """Batched float64 Kabsch over all pairs of a [m, L, 3] and b [n, L, 3] with torch.linalg.svd -> [m, n]."""
    import torch

    a = a.double() - a.double().mean(1, keepdim=True)
    b = b.double() - b.double().mean(1, keepdim=True)
    h = torch.einsum("ail,bim->ablm", a, b)
    u, s, vt = torch.linalg.svd(h)
    sign = torch.sign(torch.linalg.det(u @ vt))
    lam = s[..., 0] + s[..., 1] + sign * s[..., 2]
    msd = (a.square().sum((1, 2))[:, None] + b.square().sum((1, 2))[None, :] - 2.0 * lam) / a.shape[1]
    return msd.clamp_min(0.0).sqrt()


def run_case(name):
    import torch

    from str2str_amd import ops

    n_a, n_b, L = CASES[name]
    a = chains(n_a, L, 1)
    b = None if n_b is None else chains(n_b, L, 2)
    cols = n_a if b is None else n_b
    out = torch.empty(n_a, cols, dtype=torch.float64, device="cuda")
    kernel_ms, reps = timing_common.time_window(lambda: ops.ca_rmsd_matrix(a, b, out=out), warmup=3)
    pairs = n_a * cols
    computed = n_a * (n_a + 1) // 2 if b is None else pairs         # the self case evaluates the upper triangle and mirrors it
    rows = max(1, min(n_a, BASELINE_PAIRS // cols))
    n_rows = min(n_a, max(rows, BASELINE_PAIRS // cols // rows * rows))
    bb = a if b is None else b

    def baseline():
        for r0 in range(0, n_rows, rows):
            svd_rmsd(a[r0:r0 + rows], bb)

    svd_ms, svd_reps = timing_common.time_window(baseline, warmup=1)
    err = float((svd_rmsd(a[:rows], bb) - out[:rows]).abs().max())
    return {"case": name, "n_a": n_a, "n_b": cols, "L": L, "pairs": pairs, "kernel_ms": kernel_ms, "kernel_reps": reps,
            "svd_ms_measured": svd_ms, "svd_pairs_measured": n_rows * cols, "svd_reps": svd_reps, "svd_ms_all_pairs": svd_ms * n_a / n_rows,
            "flop": 18.0 * L * computed, "share_of_f64_matrix_peak": 18.0 * L * computed / (kernel_ms * 1e-3) / PEAK_F64_MATRIX,
            "max_abs_diff_vs_svd": err, "device": torch.cuda.get_device_name(0)}


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "ensemble_rmsd_timing.md"), CASE_TIMEOUT_S)
    if rows is None:
        return 0
    lines = ["# All-pairs minimum RMSD: s2s_ca_rmsd_matrix against batched float64 torch.linalg.svd", "",
             f"Device: {rows[0]['device']}.  `python tools/rmsd_timing.py`; device events around the whole call, mean over the repetitions.", "",
             "| case | pairs | kernel (ms) | torch.linalg.svd float64, same pairs (ms) | speed-up | share of the float64 matrix peak | max abs diff vs SVD (A) |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        scaled = "" if r["svd_pairs_measured"] == r["pairs"] else f" (timed on {r['svd_pairs_measured']} pairs, scaled)"
        lines.append(f"| {r['case']} | {r['pairs']} | {r['kernel_ms']:.3f} | {r['svd_ms_all_pairs']:.1f}{scaled} | "
                     f"{r['svd_ms_all_pairs'] / r['kernel_ms']:.0f}x | {100 * r['share_of_f64_matrix_peak']:.2f} % | {r['max_abs_diff_vs_svd']:.2e} |")
    lines += ["", "Share of peak: 2 x 9 x L flop per computed pair (the cross-covariance product alone; the self case computes the upper "
              "triangle) over the call's time, against the data sheet's 78.6 TFLOP/s float64 matrix rate.  The call also runs the prepass and "
              "one 4 x 4 Jacobi eigen-solve per pair, which the flop count leaves out.", ""]
    timing_common.write_report(out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
