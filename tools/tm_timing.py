"""Time the all-pairs TM-score kernel (s2s_ca_tm_matrix) against what a user would write today: the same algorithm -- the same seeds, 33
reweighted Kabsch steps, maximum over seeds -- in batched float64 torch on the same device.

    python tools/tm_timing.py [--out profiles/ensemble_tm_timing.md]      all cases, each in a child process under its own time limit
    python tools/tm_timing.py --case self_1000_L256 [--kernel-only]       one case, one JSON line (--kernel-only: for a profiler run)

Cases: the self matrix of R = 1000 structures at L = 35, 80 and 256.  Times are device events around the whole call, after warm-up, over
enough repetitions for a window of >= 0.5 s.  The torch baseline is timed on BASELINE_PAIRS pairs of the case's upper triangle and scaled
to all computed pairs (stated in the output); its values are compared with the kernel's on those pairs.
"Share of the float64 vector peak" = FLOP_PER_RESIDUE flop per (computed pair, seed, pass, residue) over the kernel's time against the
78.6 TFLOP/s float64 vector rate of the MI355X data sheet; the 4 x 4 eigen-solves and the duplicate lanes of short seed lists are left
out of the count.
"""
import os
import sys

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

CASES = {"self_1000_L35": (1000, 35), "self_1000_L80": (1000, 80), "self_1000_L256": (1000, 256)}
PEAK_F64_VECTOR = 78.6e12
# per residue and pass: d = R x + t - y (21), |d|^2 (5), f (3), score (1), w = f^2 (1), the 16 moments (31)
FLOP_PER_RESIDUE = 62
ITERS = 33
BASELINE_PAIRS = 2048
CASE_TIMEOUT_S = 240


def chains(n, L, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    step = torch.randn(n, L, 3, generator=g)
    step = 3.8 * step / step.norm(dim=-1, keepdim=True)
    base = step[:1].cumsum(1)
    noisy = base + torch.randn(n, L, 3, generator=g) * torch.linspace(0.05, 6.0, n)[:, None, None]     # an ensemble around one fold
    return (noisy + 100.0 * torch.rand(n, 1, 3, generator=g) - 50.0).to("cuda", torch.float32)


def seeds(L):
    out = [(0, L)]
    for div in (2, 4):
        n = max(L // div, 4)
        if n >= L:
            continue
        starts = list(range(0, L - n + 1, max(n // 2, 1)))
        out += [(s, n) for s in starts] + ([(L - n, n)] if starts[-1] + n < L else [])
    return list(dict.fromkeys(out))


def torch_tm(a, b):
    """Paired a, b [P, L, 3] -> TM [P]: the kernel's algorithm in batched float64 torch (weighted moments by one matmul per step,
    ``torch.linalg.svd`` Kabsch with the determinant fix)."""
    import torch

    a, b = a.double(), b.double()
    a, b = a - a.mean(1, keepdim=True), b - b.mean(1, keepdim=True)
    P, L = a.shape[:2]
    d0 = max(0.5, 1.24 * (L - 15.0) ** (1.0 / 3.0) - 1.8) if L > 15 else 0.5
    sd = seeds(L)
    w = torch.zeros(P, len(sd), L, dtype=torch.float64, device=a.device)
    for k, (s, n) in enumerate(sd):
        w[:, k, s:s + n] = 1.0
    table = torch.cat([torch.ones(P, L, 1, dtype=torch.float64, device=a.device), a, b, (a[..., :, None] * b[..., None, :]).reshape(P, L, 9)], -1)
    best = torch.zeros(P, dtype=torch.float64, device=a.device)
    for _ in range(ITERS):
        m = w @ table
        ca, cb = m[..., 1:4] / m[..., :1], m[..., 4:7] / m[..., :1]
        h = m[..., 7:].reshape(P, len(sd), 3, 3) - m[..., 1:4, None] * cb[..., None, :]
        u, _, vt = torch.linalg.svd(h)
        u = torch.cat([u[..., :2], u[..., 2:] * torch.sign(torch.linalg.det(u @ vt))[..., None, None]], -1)
        rot = (u @ vt).transpose(-1, -2)
        t = cb - (rot @ ca[..., None])[..., 0]
        d = a[:, None] @ rot.transpose(-1, -2) + t[..., None, :] - b[:, None]
        f = 1.0 / (1.0 + d.square().sum(-1) / (d0 * d0))
        best = torch.maximum(best, f.mean(-1).max(1).values)
        w = f * f
    return best


def run_case(name, kernel_only=False):
    import torch

    from str2str_amd import ops

    n, L = CASES[name]
    a = chains(n, L, 1)
    out = torch.empty(n, n, dtype=torch.float64, device="cuda")
    kernel_ms, reps = timing_common.time_window(lambda: ops.ca_tm_matrix(a, out=out), warmup=2)
    computed = n * (n + 1) // 2                               # the self case evaluates i <= j and mirrors
    flop = float(FLOP_PER_RESIDUE) * computed * len(seeds(L)) * (ITERS + 1) * L
    res = {"case": name, "n": n, "L": L, "pairs": n * n, "computed_pairs": computed, "seeds": len(seeds(L)), "kernel_ms": kernel_ms,
           "kernel_reps": reps, "flop": flop, "share_of_f64_vector_peak": flop / (kernel_ms * 1e-3) / PEAK_F64_VECTOR,
           "device": torch.cuda.get_device_name(0)}
    if kernel_only:
        return res
    i, j = torch.triu_indices(n, n, 1, device="cuda")
    pick = torch.randperm(i.numel(), generator=torch.Generator().manual_seed(3))[:BASELINE_PAIRS].to("cuda")
    i, j = i[pick], j[pick]
    torch_ms, torch_reps = timing_common.time_window(lambda: torch_tm(a[i], a[j]), warmup=1)
    res.update({"torch_ms_measured": torch_ms, "torch_pairs_measured": int(i.numel()), "torch_reps": torch_reps,
                "torch_ms_all_pairs": torch_ms * computed / i.numel(), "max_abs_diff_vs_torch": float((torch_tm(a[i], a[j]) - out[i, j]).abs().max()),
                "mean_tm": float(out[i, j].mean())})
    return res


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "ensemble_tm_timing.md"), CASE_TIMEOUT_S, kernel_only=True)
    if rows is None:
        return 0
    lines = ["# All-pairs TM-score: s2s_ca_tm_matrix against the same algorithm in batched float64 torch", "",
             f"Device: {rows[0]['device']}.  `python tools/tm_timing.py`; device events around the whole call, mean over the repetitions (measured).", "",
             "| case | pairs (computed) | seeds | kernel (ms) | torch float64, same algorithm (ms) | ratio | share of the float64 vector peak | max abs diff vs torch |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['pairs']} ({r['computed_pairs']}) | {r['seeds']} | {r['kernel_ms']:.2f} | {r['torch_ms_all_pairs']:.0f} (timed on "
                     f"{r['torch_pairs_measured']} pairs: {r['torch_ms_measured']:.1f} ms, scaled) | {r['torch_ms_all_pairs'] / r['kernel_ms']:.0f}x | "
                     f"{100 * r['share_of_f64_vector_peak']:.1f} % | {r['max_abs_diff_vs_torch']:.1e} |")
    lines += ["", f"Share of peak: {FLOP_PER_RESIDUE} flop per (computed pair, seed, pass, residue), {ITERS} evaluations plus the seeding pass, over the "
              "call's time, against the data sheet's 78.6 TFLOP/s float64 vector rate.  The count leaves out one 4 x 4 Jacobi eigen-solve per "
              "(pair, seed, evaluation) and the staging, and the lanes that repeat the whole-chain seed where the list has fewer than 16 seeds.", ""]
    timing_common.write_report(out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
