"""Time the contact kernels (s2s_ca_contact_map, s2s_ca_native_q) against what a user would write today: the same definitions -- float64
squared distances against the squared cutoff; the hard and the soft Q with one sqrt and one exp per (entry, structure) -- in batched float64
torch on the same device, the map in chunks of structures that fit memory.

    python tools/contacts_timing.py [--out profiles/contacts_timing.md]      all cases, each in a child process under its own time limit
    python tools/contacts_timing.py --case map_10000_L256 [--kernel-only]     one case, one JSON line (--kernel-only: for a profiler run)

Cases: the contact map of 10 000 structures of 256 residues and of 20 000 of 64 (cutoff 8 A, min_seq_sep 3), and Q of 10 000 structures of
256 residues against the native list of the unperturbed chain (cutoff 8 A, min_seq_sep 4, beta 5 / A, lam 1.2).  The structures are the
noisy copies of tools/lddt_timing.py (Gaussian, 0.05 .. 6 A, of the CA trace of tests/golden/pdb/lambda.pdb tiled to the length).  Every
repetition is timed on its own with device events around the whole call, after warm-up; all of them are written out.  There is no
pass/fail condition: the report records what the run gives.
The kernel's work is counted from the shapes: the map evaluates (eligible pairs) x (structures), each two points (24 B as float32; the
kernel holds them widened) from LDS and 8 float64 operations (three differences, three products, two sums) and one comparison; Q evaluates
(list entries) x (structures), each the same squared distance plus one sqrt and one exp.
"""
import os
import sys

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

CASES = {"map_10000_L256": ("map", 10000, 256), "map_20000_L64": ("map", 20000, 64), "q_10000_L256": ("q", 10000, 256)}
CUTOFF, MAP_SEP, NATIVE_SEP, BETA, LAM = 8.0, 3, 4, 5.0, 1.2
REPEATS = 5
TORCH_CHUNK_BYTES = 1 << 30          # the [chunk, L, L, 3] float64 difference tensor of the torch restatement of the map
CASE_TIMEOUT_S = 300
PEAK_F64_VECTOR = 78.6e12            # the data sheet's float64 vector rate


def torch_contact_counts(x, cutoff=CUTOFF, sep=MAP_SEP):
    """x [R, L, 3] float32 -> counts [L, L] int32, symmetric: the definition, batched over chunks of structures."""
    import torch

    R, L = x.shape[:2]
    counts = torch.zeros(L, L, dtype=torch.int64, device=x.device)
    rows = max(1, TORCH_CHUNK_BYTES // (24 * L * L))
    for r0 in range(0, R, rows):
        xd = x[r0:r0 + rows].double()
        d = xd[:, :, None, :] - xd[:, None, :, :]
        v = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        counts += (v < cutoff * cutoff).sum(0)
    upper = torch.triu(counts, diagonal=sep)
    return (upper + upper.T).to(torch.int32)


def torch_native_q(x, pairs, d0, beta=BETA, lam=LAM):
    """x [R, L, 3] float32, pairs [n, 2], d0 [n] -> (q_soft [R], hits [R]): the definition, batched."""
    xd = x.double()
    d = xd[:, pairs[:, 0].long()] - xd[:, pairs[:, 1].long()]
    v = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    b = lam * d0
    return (1.0 / (1.0 + (beta * (v.sqrt() - b)).exp())).sum(1) / len(pairs), (v < b * b).sum(1)


def run_case(name, kernel_only=False):
    import torch

    import lddt_timing
    from str2str_amd import ops

    kind, n, L = CASES[name]
    x = lddt_timing.ensemble(n, L, 1)
    res = {"case": name, "kind": kind, "n": n, "L": L, "device": torch.cuda.get_device_name(0)}
    if kind == "map":
        res["kernel_ms"] = timing_common.time_repetitions(lambda: ops.ca_contact_map(x, CUTOFF, MAP_SEP), REPEATS, warmup=2)
        if kernel_only:
            return res
        res["torch_ms"] = timing_common.time_repetitions(lambda: torch_contact_counts(x), REPEATS, warmup=1)
        got, want = ops.ca_contact_map(x, CUTOFF, MAP_SEP)[0], torch_contact_counts(x)
        res.update({"entries_that_differ": int((got != want).sum()), "evaluations": float(n) * (L - MAP_SEP) * (L - MAP_SEP + 1) / 2,
                    "contacts_per_structure": float(got.sum()) / 2 / n, "operations_per_evaluation": 9})
    else:
        native = torch.as_tensor(lddt_timing.chain(L)).to("cuda", torch.float32)
        pairs, d0 = ops.ca_native_contacts(native, CUTOFF, NATIVE_SEP)
        res["kernel_ms"] = timing_common.time_repetitions(lambda: ops.ca_native_q(x, pairs, d0, BETA, LAM), REPEATS, warmup=2)
        res["list_entries"] = int(pairs.shape[0])
        if kernel_only:
            return res
        res["torch_ms"] = timing_common.time_repetitions(lambda: torch_native_q(x, pairs, d0), REPEATS, warmup=1)
        (q_soft, _, hits), (want_soft, want_hits) = ops.ca_native_q(x, pairs, d0, BETA, LAM), torch_native_q(x, pairs, d0)
        res.update({"entries_that_differ": int((hits != want_hits).sum()), "max_abs_diff_soft_q": float((q_soft - want_soft).abs().max()),
                    "evaluations": float(n) * pairs.shape[0], "mean_soft_q": float(q_soft.mean()), "operations_per_evaluation": 15})
    best = min(res["kernel_ms"]) * 1e-3
    res.update({"evaluations_per_s": res["evaluations"] / best, "lds_bytes_per_s": 24.0 * res["evaluations"] / best})
    return res


def _ms(xs):
    return ", ".join(f"{x:.2f}" for x in xs)


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "contacts_timing.md"), CASE_TIMEOUT_S, kernel_only=True)
    if rows is None:
        return 0
    lines = ["# Contacts: s2s_ca_contact_map and s2s_ca_native_q against the same definitions in batched float64 torch", "",
             f"Device: {rows[0]['device']}.  `python tools/contacts_timing.py`; every repetition between its own pair of device events around the "
             f"whole call, after warm-up (measured).  Inputs: noisy copies (0.05 .. 6 A) of the CA trace of `tests/golden/pdb/lambda.pdb` tiled to "
             f"the length.  Map: cutoff {CUTOFF} A, min_seq_sep {MAP_SEP}; the torch restatement walks the structures in chunks whose "
             f"[chunk, L, L, 3] float64 difference tensor is {TORCH_CHUNK_BYTES >> 20} MiB.  Q: the native list of the unperturbed chain (cutoff "
             f"{CUTOFF} A, min_seq_sep {NATIVE_SEP}), beta {BETA} / A, lam {LAM}; the list pass is outside the timed call.  No pass/fail "
             f"condition: this is the record of one run.", "",
             "| case | kernel, every repetition (ms) | torch float64, every repetition (ms) | fastest torch / fastest kernel | integer entries that differ | note |",
             "|---|---|---|---|---|---|"]
    for r in rows:
        note = (f"{r['contacts_per_structure']:.0f} contacts per structure" if r["kind"] == "map" else
                f"{r['list_entries']} list entries; max abs diff of the soft Q vs torch {r['max_abs_diff_soft_q']:.1e}; mean soft Q {r['mean_soft_q']:.4f}")
        lines.append(f"| {r['case']} | {_ms(r['kernel_ms'])} | {_ms(r['torch_ms'])} | {min(r['torch_ms']) / min(r['kernel_ms']):.1f} | "
                     f"{r['entries_that_differ']} | {note} |")
    lines += ["", "What the fastest repetition of the kernel sustains (derived from the measured time and the counted work: one evaluation = one "
              "eligible pair, or one list entry, of one structure = 24 B of coordinates from LDS and 8 float64 operations and a comparison; Q adds "
              "a scaling, a subtraction, a sqrt, an exp, an addition and a division, each counted as one operation; staging, the mirror pass "
              "and the reductions are inside the time):", "",
              "| case | evaluations | evaluations / s | LDS coordinates (TB/s) | share of the float64 vector peak (counted operations, 78.6 TFLOP/s) |",
              "|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['evaluations']:.3e} | {r['evaluations_per_s']:.3e} | {r['lds_bytes_per_s'] / 1e12:.2f} | "
                     f"{100 * r['operations_per_evaluation'] * r['evaluations_per_s'] / PEAK_F64_VECTOR:.1f} % |")
    lines.append("")
    timing_common.write_report(out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
