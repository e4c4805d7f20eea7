"""Time the TICA path (metrics.tica / metrics.tica_project) split into its parts, next to the host path it replaces.

    python tools/tica_timing.py [--out profiles/tica_timing.md]      all cases, each in a child process under its own time limit
    python tools/tica_timing.py --case tica_10000_L35                one case, one JSON line

Cases: trajectories of 10 000 and of 100 000 frames of chains of 35, 58 and 80 residues (D = 595, 1596 and 3160 CA distances), lag 20.
The frames are the CA atoms of the noisy copies of the lambda-repressor backbone of tools/timing_common.py cut to the length: the
arithmetic does not depend on the values.  Timed, each repetition between its own pair of device events after warm-up: the features
(s2s_ca_pairwise_distances), the reversible mean (s2s_lagged_mean), the two covariances (the prepass, the product kernel and, where the
pairs are split into groups, the reduction of s2s_lagged_covariances) and the projection of the trajectory onto two components
(s2s_feature_project).  Timed once with the wall clock: the host tail on the device's covariances (the copy of both matrices and
metrics._tica_from_covariances: two symmetric eigenproblems), and the host path of the parent commit, metrics.tica_fit on the same
features.  With STR2STR_TICA_ONE_GROUP_LIB naming a build of the library whose S2S_TICA_WAVE_SLOTS is 1 (tools/build_variant.sh with
UNIT=ensemble_tica and -DS2S_TICA_WAVE_SLOTS=1: every shape then takes G = 1) the covariances of that library are timed in the same
process, interleaved with the regular one, and compared byte for byte where both take one group.  There is no pass/fail condition: the
report records what the run gives."""
import os
import sys
import time

import timing_common

ROOT = timing_common.ROOT
sys.path.insert(0, ROOT)

LAG = 20
CASES = {f"tica_{T}_L{L}": (T, L) for T in (10000, 100000) for L in (35, 58, 80)}
REPEATS = 3
CASE_TIMEOUT_S = 900


def covariances_of(lib, f, mean, lag, groups):
    """s2s_lagged_covariances of the library ``lib``, which divides the pairs into ``groups`` groups, with the wrapper's default workspace."""
    import torch

    from str2str_amd.ops import binding, ensemble

    T, D = f.shape
    blocks = -(-D // 48)
    step = max(4, ensemble.PCA_WORKSPACE_BYTES // (8 * 2 * 48 * blocks) // groups // 4 * 4)
    partials = groups * 2 * (blocks * (blocks + 1) // 2) * 2304 if groups > 1 else 0
    ws = torch.empty(2 * blocks * 48 * groups * step + partials, dtype=torch.float64, device=f.device)
    c00, c0t = (torch.empty(D, D, dtype=torch.float64, device=f.device) for _ in range(2))
    binding._check(lib.s2s_lagged_covariances(binding._p(f), T, D, lag, binding._p(mean), binding._p(c00), binding._p(c0t), binding._p(ws),
                                              ws.numel(), binding._stream()), "s2s_lagged_covariances")
    return c00, c0t


def run_case(name):
    import torch

    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    T, L = CASES[name]
    atoms, _, _ = timing_common.lambda_backbone_ensemble(T, L)
    ca = atoms[:, :, 1].contiguous()
    del atoms
    features_ms = timing_common.time_repetitions(lambda: ops.ca_pairwise_distances(ca, 1), REPEATS, warmup=1)
    f = ops.ca_pairwise_distances(ca, 1)
    D = f.shape[1]
    G, group = ops.tica_groups(T - LAG, D)
    mean_ms = timing_common.time_repetitions(lambda: ops.lagged_mean(f, LAG), REPEATS, warmup=1)
    mean = ops.lagged_mean(f, LAG)
    cov_ms = timing_common.time_repetitions(lambda: ops.lagged_covariances(f, mean, LAG), REPEATS, warmup=1)
    one_group_ms, one_group_same = None, None
    variant = os.environ.get("STR2STR_TICA_ONE_GROUP_LIB")
    if variant:
        one = ops.load_library(variant)
        one_group_ms, again_ms = [], []
        for _ in range(REPEATS + 1):                         # interleaved A/B in this process; the first round is the warm-up
            one_group_ms += timing_common.time_repetitions(lambda: covariances_of(one, f, mean, LAG, 1), 1, warmup=0)
            again_ms += timing_common.time_repetitions(lambda: ops.lagged_covariances(f, mean, LAG), 1, warmup=0)
        one_group_ms, cov_ms = one_group_ms[1:], again_ms[1:]
        if G == 1:
            one_group_same = all(torch.equal(a, b) for a, b in zip(covariances_of(one, f, mean, LAG, 1), ops.lagged_covariances(f, mean, LAG)))
    c00, c0t = ops.lagged_covariances(f, mean, LAG)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    proj, lam, rank = metrics._tica_from_covariances(c00.cpu().numpy(), c0t.cpu().numpy(), 2, 1e-6)
    tail_s = time.perf_counter() - t0
    comps = torch.as_tensor(proj.T.copy(), device=f.device)
    project_ms = timing_common.time_repetitions(lambda: ops.feature_project(f, mean, comps), REPEATS, warmup=1)
    symmetric = bool(torch.equal(c00, c00.T) and torch.equal(c0t, c0t.T))
    del c00, c0t
    f_host = f.cpu().numpy()
    t0 = time.perf_counter()
    _, host_proj = metrics.tica_fit(f_host, LAG, dim=2)
    host_s = time.perf_counter() - t0
    blocks = -(-D // 48)
    tri = blocks * (blocks + 1) // 2
    return {"case": name, "T": T, "L": L, "D": D, "device": torch.cuda.get_device_name(0), "groups": G, "group_pairs": group, "blocks": tri,
            "features_ms": features_ms, "mean_ms": mean_ms, "cov_ms": cov_ms, "one_group_ms": one_group_ms, "one_group_same": one_group_same,
            "project_ms": project_ms, "tail_s": tail_s, "host_s": host_s, "rank": int(rank), "eigenvalues": [float(v) for v in lam],
            "flops": 2.0 * 4 * (T - LAG) * (48 * 48) * tri, "symmetric": symmetric,
            "components_vs_host": float(abs(proj - host_proj).max() / abs(host_proj).max())}


def main():
    rows, out = timing_common.collect(__file__, CASES, run_case, os.path.join(ROOT, "profiles", "tica_timing.md"), CASE_TIMEOUT_S)
    if rows is None:
        return 0
    fmt = lambda ts: "-" if ts is None else ", ".join(f"{t:.2f}" for t in ts)   # noqa: E731
    lines = ["# TICA: time-lagged covariances on the device, the eigenproblems on the host", "",
             f"Device: {rows[0]['device']}.  `python tools/tica_timing.py`; every repetition of a device part between its own pair of device "
             f"events, after warm-up; the host parts once with the wall clock (all measured).  Lag {LAG}.  Inputs: the CA atoms of noisy copies "
             "(0.02 .. 1 A) of the backbone of `tests/golden/pdb/lambda.pdb` cut to the length, featurised with their CA distances.  No "
             "pass/fail condition: this is the record of one run.", "",
             "| case | D | features (ms) | mean (ms) | covariances (ms) | projection, 2 components (ms) | host tail: copies + two eigh (s) | "
             "parent's host path: tica_fit on the same features (s) | rank | components against tica_fit's (relative) |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['D']} | {fmt(r['features_ms'])} | {fmt(r['mean_ms'])} | {fmt(r['cov_ms'])} | {fmt(r['project_ms'])} | "
                     f"{r['tail_s']:.2f} | {r['host_s']:.2f} | {r['rank']} | {r['components_vs_host']:.1e} |")
    lines += ["", "The k-split (the pairs divided into G groups where the upper triangle has fewer blocks than the device has wave slots) against "
              "one group, the same shapes through a build of the library with `S2S_TICA_WAVE_SLOTS` 1, interleaved in the same process; and what "
              "the fastest call sustains (derived from the measured time and the counted work: 4 x 48 x 48 multiply-adds per pair and "
              "upper-triangle block; the prepass and the reduction are inside the time):", "",
              "| case | upper-triangle blocks | G | pairs per group | covariances (ms) | one group (ms) | same bytes where G = 1 | float64 flop per call | "
              "float64 flop / s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['blocks']} | {r['groups']} | {r['group_pairs']} | {fmt(r['cov_ms'])} | {fmt(r['one_group_ms'])} | "
                     f"{'-' if r['one_group_same'] is None else r['one_group_same']} | {r['flops']:.3e} | {r['flops'] / (min(r['cov_ms']) * 1e-3):.3e} |")
    lines.append("")
    timing_common.write_report(out, lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
