"""The forward-backward diffusion sampler (device-resident loop).

This is the closure ``forward_backward`` of the reference's ``DiffusionLitModule.predict_step``
(src/models/diffusion_module.py:260-334) with the same schedule semantics:
``n = int(num_timesteps*T)``, ``dt = 1/n`` (not the spacing of ``ts``), ``ts = linspace(min_t, T, n)[::-1]``,
one extra network evaluation for self-conditioning, and the last step (``t == min_t``) returning the
x0 prediction itself.  Differences in HOW:
  * all per-step scalars (sigma bin, g(t)^2, exp(-beta/2), ...) are computed on the host once per
    trajectory; the loop body is network forward -> ONE fused SE(3) kernel, with no device->host sync;
  * the backbone projection runs once at the end (the reference recomputes it every forward and
    throws the result away, denoising_ipa.py:197-201);
  * the default arithmetic (split-f16 matrix products, str2str_amd/arith.py) has f16's RANGE: its kernels raise a device flag
    when a value they split reaches 2^15; the flag is read once per chunk, where the loop synchronises anyway, and a flagged
    chunk is re-run from its starting frames (same noise) on the exact fp32 kernels -- after which the network stays there;
  * replicas can be sharded over ranks (``shard=(rank, world)``): noise for the WHOLE chunk is drawn
    on every rank from the same host generator state and sliced, so the union over ranks equals the
    single-process result sample for sample ("parity" RNG mode).  ``rng="device"`` instead draws
    nothing on the host inside the loop (throughput mode; different noise stream).

Shape of the module: every driver (``forward_backward``: one chunk, ``forward_backward_chunks``: the chunks of one t_delta,
``forward_backward_deltas`` / ``iter_forward_backward_deltas``: the t_deltas of a target) is an adapter over the same three steps:
  * ``_batch_plan``: the reference's stream of (t_delta, chunk) entries, t_delta-major and chunk-minor, cut into BATCHES of consecutive
    entries (several whole t_deltas | a run of chunks of one t_delta | one entry) by ``merge_delta_groups`` / ``merge_chunk_groups``;
  * ``_draw_entries``: THE walk over the host noise stream -- per entry the whole chunk's start frames, then its 2 (n - 1) step
    draws, burnt right there or (the last entry of a batch only) deferred into the loop;
  * ``_sample_batch`` -> ``_denoise_pass``: THE loop, under the range guard, over one group of samples per t_delta of the batch;
    a batch with one schedule takes the shared-row form (HIP-graph eligible), one with several the per-sample form.
``denoise_loop`` (already expanded features, one schedule) and ``sample_mixed_lengths`` (padded rows) enter at the pass.
"""
from __future__ import annotations

import contextlib
import logging
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import ops
from .arith import FAMILIES, net_arith, use_arith
from .common.all_atom import compute_backbone
from .common.rigid_utils import Rigid

_REPEAT_KEYS = ("aatype", "residue_mask", "fixed_mask", "residue_idx", "torsion_angles_sin_cos")
_log = logging.getLogger("str2str_amd.sampler")
# A network evaluation is ~165 kernel launches (profiles/r02m_eval_sequence.md).  For tiny chunks (<= 64 Ki pairs, e.g. 64 replicas
# of a 20-residue peptide) the GPU finishes them faster than the host can issue them, so the evaluation is captured once into a
# HIP graph and replayed every step: 1.7x there, bit-identical output; larger chunks are GPU-bound (the host already runs ahead)
# and capture would only add its three warm-up evaluations (measured 0.92-0.97x).  S2S_HIP_GRAPH=0 / 1 forces eager / graph.
_GRAPH_MAX_PAIRS = 1 << 16
_GRAPH_MIN_STEPS = 16


class _GraphedNet:
    """One captured network evaluation on static input buffers (rigids_t, sc_ca_t, t_img); outputs are static too."""

    def __init__(self, net, feats):
        self.feats = dict(feats)
        self.static = tuple(k for k in ("rigids_t", "sc_ca_t", "t_img") if k in feats)
        for k in self.static:
            self.feats[k] = feats[k].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on a side stream (caches, BLAS workspaces), as graph capture requires
            for _ in range(2):
                _net_eval(net, self.feats, True)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = _net_eval(net, self.feats, True)
        # The captured kernels hold raw pointers to every tensor the evaluation read.  Those allocated INSIDE the capture live in the
        # graph's private pool; the ones built by the warm-up outside it must be kept alive by THIS object, because their only other
        # owner is a single-slot cache (layers.DerivedCache) that the next evaluation of another shape or target overwrites:
        # per-target tables, mask terms, constant rows, packed / derived weights.
        self._pinned = _graph_read_tensors(net)

    def __call__(self, feats):
        for k in self.static:
            self.feats[k].copy_(feats[k])
        self.graph.replay()
        return self.out


def _graph_read_tensors(net):
    """Every tensor (values and their sources) held by the ``DerivedCache`` slots of the network's modules -- by construction all the
    derived device tensors that module state holds."""
    from .models.net.layers import DerivedCache

    def tensors(x, out):
        if torch.is_tensor(x):
            out.append(x)
        elif isinstance(x, dict):
            for v in x.values():
                tensors(v, out)
        elif isinstance(x, (list, tuple)):
            for v in x:
                tensors(v, out)
        return out

    keep = []
    for m in net.modules():
        for v in vars(m).values():
            if isinstance(v, DerivedCache):
                tensors(v.held(), keep)
    return keep


def _net_eval(net, feats, defer_psi: bool):
    """One evaluation inside the loop: the psi blend is deferred to the last step where the network supports it."""
    if defer_psi and hasattr(net, "blend_psi"):
        return net(feats, as_tensor_7=False, defer_psi_blend=True)
    return net(feats, as_tensor_7=False)


_GRAPH_CACHE = {}   # (net id, parameter versions, b, N, feature bytes) -> _GraphedNet; a few entries (one per chunk shape)
_GRAPH_CACHE_MAX = 4


def _graph_key(net, feats, b, N):
    import hashlib

    h = hashlib.sha1()
    for k in sorted(feats):
        v = feats[k]
        if k in ("rigids_t", "sc_ca_t", "t_img", "t") or not torch.is_tensor(v):
            continue  # per-step inputs are copied into the static buffers at every replay
        h.update(k.encode()); h.update(str(tuple(v.shape)).encode()); h.update(v.detach().cpu().numpy().tobytes())
    # which kernels were captured: every switch the module classes declare (``launch_switches``: arithmetic, block exponents, folded
    # attention operands, padding semantics, ...), per module in module order -- a mixed network has many forms
    modes = tuple((type(m).__name__, a, getattr(m, a)) for m in net.modules()
                  for a in getattr(type(m), "launch_switches", ()) + getattr(type(m), "launch_modes", ()))
    return (id(net), sum(p._version for p in net.parameters()), b, N, modes, h.hexdigest())


def _maybe_graph(net, feats, b, N, trace, n_steps):
    mode = os.environ.get("S2S_HIP_GRAPH", "auto")
    if mode == "0" or trace is not None or ops.KernelTimer.active is not None:
        return None
    if mode != "1" and (b * N * N > _GRAPH_MAX_PAIRS or n_steps < _GRAPH_MIN_STEPS):
        return None
    key = _graph_key(net, feats, b, N)   # chunks / t_deltas of one target share the capture (same static features)
    hit = _GRAPH_CACHE.get(key)
    if hit is not None:
        return hit
    try:
        g = _GraphedNet(net, feats)
    except ops.HipLibraryError:
        raise                            # a kernel / ABI error is an error, not a capture problem
    except RuntimeError as e:            # capture itself is an optimisation: fall back to eager launches
        _log.warning("HIP graph capture failed (%s); continuing with eager launches", repr(e)[:200])
        torch.cuda.synchronize()
        return None
    if len(_GRAPH_CACHE) >= _GRAPH_CACHE_MAX:
        _GRAPH_CACHE.pop(next(iter(_GRAPH_CACHE)))
    _GRAPH_CACHE[key] = g
    return g


def schedule(t_delta: float, num_timesteps: int, min_t: float):
    T = t_delta if t_delta > 0 else 1.0
    n = int(float(num_timesteps) * T)
    return T, n, 1.0 / n, np.linspace(min_t, T, n)[::-1]


def shard_range(total: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous replica range of ``rank``: ceil split, rank-major order == replica order."""
    per = -(-total // world)
    lo = min(total, rank * per)
    return lo, min(total, lo + per)


def rank_chunk_slices(n_replica: int, replica_per_batch: int, rank: int, world: int):
    """How ``rank`` walks the reference's replica chunks (diffusion_module.py:341-351: ``n_replica`` split into chunks of
    ``replica_per_batch``, the unit of its host noise stream) when the WHOLE replica range is sharded over ``world`` ranks:
    -> [(chunk_size, lo, hi)] per chunk, (lo, hi) = the part of that chunk inside this rank's contiguous range
    ``shard_range(n_replica, rank, world)`` ((0, 0) when the chunk lies outside it).  Rank-major concatenation of the
    sampled slices is the single-process replica order."""
    my_lo, my_hi = shard_range(n_replica, rank, world)
    sizes = [replica_per_batch] * (n_replica // replica_per_batch)
    if n_replica % replica_per_batch > 0:
        sizes.append(n_replica % replica_per_batch)
    out, c0 = [], 0
    for bsz in sizes:
        lo, hi = max(my_lo, c0) - c0, min(my_hi, c0 + bsz) - c0
        out.append((bsz, lo, hi) if hi > lo else (bsz, 0, 0))
        c0 += bsz
    return out


@torch.no_grad()
def denoise_loop(net, diffuser, feats: dict, rigids_t: torch.Tensor, ts, dt: float, *, min_t: float,
                 noise_scale: float = 1.0, probability_flow: bool = True, self_conditioning: bool = True,
                 center_mode: int = 1, host_noise=None, trace: Optional[list] = None):
    """The loop body of forward_backward over ALREADY EXPANDED per-sample features (every tensor has the
    sample dimension b) starting from the noised frames ``rigids_t`` [b,N,7]: 1 self-conditioning evaluation,
    then per step  network -> fused SE(3) step, last step returns the x0 prediction.  ``host_noise()`` (optional)
    returns the (z_rot, z_trans) float64 [b,N,3] device tensors of a step or None.  -> (atom37, final rigids7, psi).

    Range guard: in the split-f16 arithmetic the pass runs with its device's range flag cleared; if a kernel raised it (an
    activation reached 2^15 -- f16 tops out at 65504) or the result is not finite, the SAME chunk (same starting frames, same
    noise) is run again with ONLY the kernel families that raised it (str2str_amd/arith.py: node stream, edge transition, edge
    embedding, IPA) on their exact fp32 kernels; a warning is logged once per family and those families stay in fp32 for later
    chunks (``net.range_fallback`` = the set of demoted families) -- one out-of-range activation in, say, the encoder attention no
    longer costs the edge transitions (73 % of the step) their 3x.  One flag read per chunk, where the loop synchronises anyway.
    The edge transitions -- the family whose demotion would cost 2x of the whole step -- are first given a BLOCK EXPONENT instead
    (``EdgeTransition.prescale_exp`` 0 -> 5 -> 10 -> 15: the kernel keeps its hidden activations as planes of 2^-e x the value, exact
    and at the same speed, include/str2str_hip.h) and only go to fp32 when 2^30 is not enough; ``net.range_prescale`` records it."""
    if float(ts[-1]) != min_t:
        raise ValueError(f"the schedule ends at t = {float(ts[-1])}, not at min_t = {min_t}: its last evaluation is the sample")
    return _guarded_pass(net, diffuser, [dict(rigids_t=rigids_t, ts=ts, dt=dt, feats=feats)], noise_scale=noise_scale,
                         probability_flow=probability_flow, self_conditioning=self_conditioning, center_mode=center_mode,
                         host_noise=host_noise, trace=trace)[0]


def _guarded_pass(net, diffuser, groups, *, probability_flow: bool, host_noise, trace: Optional[list] = None, **kw):
    """``_denoise_pass`` over ``groups`` under the range guard (``denoise_loop``) -> [(atom37, rigids7, psi)] per group."""
    def run_pass():
        return _denoise_pass(net, diffuser, groups, probability_flow=probability_flow, host_noise=host_noise, trace=trace, **kw)

    return _range_guarded(net, run_pass, groups[0]["rigids_t"].device, host_draws=host_noise is not None,
                          device_draws=host_noise is None and not probability_flow, trace=trace)[0]


def _range_guarded(net, run_pass, device, *, host_draws: bool, device_draws: bool, trace: Optional[list] = None):
    """``run_pass()`` (one complete pass over a batch of trajectories from their starting frames -> a tuple whose element 1 holds the
    final frames) under the range guard described in ``denoise_loop``: repeated with the flagged kernel families demoted (or the
    edge transitions' block exponent raised) until no flag is raised; every repetition sees the same noise (generator states
    restored)."""
    if net_arith(net) == "f32":
        out = run_pass()
        _require_finite(out[1], "fp32")
        return out
    demoted = set(getattr(net, "range_fallback", None) or ())
    rng_state = torch.cuda.get_rng_state(device) if device_draws else None
    # Host noise (parity mode) comes from the global CPU generator (_sample_batch.host_noise): a replay re-draws it from the
    # generator state saved here -- nothing is recorded (the draws of a long SDE trajectory at b = 128, N = 512 are ~0.6 GB), and
    # every pass leaves the generator where one completed pass leaves it.
    host_state = torch.get_rng_state() if host_draws else None
    while True:
        if host_state is not None:
            torch.set_rng_state(host_state)
        ops.range_flag_reset(device)
        try:
            with use_arith(net, "f32", families=tuple(demoted)):
                out = run_pass()
            finite = bool(torch.isfinite(out[1]).all())     # (the synchronisation point of the chunk)
            bits = ops.range_flag_read(device)
            if bits == 0 and finite:
                return out
            new = set(ops.range_families(bits)) - demoted
            why = f"an activation left f16's safe range in the split-f16 kernels ({ops.range_flag_names(bits)}{'' if finite else '; non-finite frames'})"
            if "edge_transition" in new:
                e_now = _raise_edge_prescale(net)
                if e_now:
                    new.discard("edge_transition")
                    _log.warning("range guard: %s; the edge transitions keep the split-f16 kernel with a block exponent of %d on their "
                                 "hidden activations (planes of 2^-%d x the value: exact, same speed; usable range 2^%d) -- re-running this chunk",
                                 why, e_now, e_now, 15 + e_now)
                    net.range_prescale = {"edge_transition": e_now}
                    if not new:
                        if trace is not None:
                            del trace[:]
                        if rng_state is not None:
                            torch.cuda.set_rng_state(rng_state, device)
                        continue
        except ops.WeightRangeError as e:   # |32 w| >= 65504: the weights themselves cannot be packed for the f16 kernels
            new = set(FAMILIES) - demoted
            if not new:     # every family already runs its exact fp32 kernels (which pack nothing): not a range event, the caller's error
                raise
            why = f"a weight does not fit the split-f16 packing ({e})"
        if not new:
            if len(demoted) == len(FAMILIES):
                _require_finite(out[1], "fp32 (range fallback)")
                return out
            new = set(FAMILIES) - demoted   # non-finite frames without a flag: nothing names a family, everything goes exact
        demoted |= new
        _log.warning("range guard: %s; re-running this chunk with the %s kernels on exact fp32 and keeping them there (now in fp32: %s; "
                     "S2S_ARITH=f32 starts everything in fp32)", why, " + ".join(sorted(new)), ", ".join(sorted(demoted)))
        net.range_fallback = frozenset(demoted)
        if trace is not None:
            del trace[:]
        if rng_state is not None:
            torch.cuda.set_rng_state(rng_state, device)


def _raise_edge_prescale(net, step: int = 5, top: int = 15) -> int:
    """Next block exponent of the network's EdgeTransition kernels (all of them: the guard's flag names the family); 0 = none left."""
    mods = [m for m in net.modules() if hasattr(m, "prescale_exp") and getattr(m, "arith", None) == "f16x3"]
    cur = max((int(m.prescale_exp) for m in mods), default=top)
    if not mods or cur >= top:
        return 0
    for m in mods:
        m.prescale_exp = min(cur + step, top)
    return min(cur + step, top)


def _require_finite(rigids7, what):
    if not bool(torch.isfinite(rigids7).all()):
        raise ops.HipLibraryError(f"non-finite frames at the end of the trajectory in the {what} arithmetic: the network itself "
                                  "overflows fp32 on this input (weights / checkpoint?)")


@contextlib.contextmanager
def _backbone_deferred(net):
    """The network's own backbone projection off inside the block (its result is unused in the loop; ``_denoise_pass`` projects once)."""
    keep = getattr(net, "backbone_in_forward", None)
    if keep is not None:
        net.backbone_in_forward = False
    try:
        yield
    finally:
        if keep is not None:
            net.backbone_in_forward = keep


def _denoise_pass(net, diffuser, groups, *, noise_scale: float, probability_flow: bool, self_conditioning: bool, center_mode: int,
                  host_noise, trace: Optional[list]):
    """One pass of the loop in the network's current arithmetic (see ``denoise_loop``) over ``groups`` = [dict(rigids_t [b_k,N,7],
    ts (descending, ending at min_t), dt, feats: ALREADY EXPANDED per-sample features [b_k, ...])] in output order: one group per
    schedule (the t_deltas of the reference's inference block), ONE batch.  The trajectories are aligned at their END: group k
    (n_k steps) joins at global step n_max - n_k, after its own self-conditioning evaluation on an empty ``sc_ca_t``, and the batch's
    features are the concatenation of its members' -- so each sample sees exactly the evaluations of a run of its group alone (the
    kernels are batch-invariant).  ``host_noise()`` is called once per global step that is followed by an SE(3) step.
    -> ([(atom37, rigids7, psi)] per group, rigids7 of the whole batch)."""
    device = groups[0]["rigids_t"].device
    N = groups[0]["rigids_t"].shape[1]
    emb = net.embedder
    order = sorted(range(len(groups)), key=lambda k: -len(groups[k]["ts"]))     # join order (stable: equal lengths keep output order)
    n_max = len(groups[order[0]]["ts"])
    # THE choice of form, by the number of schedules in the batch.  One: the timestep image is one row [512] of the schedule's table
    # for the whole batch, the step parameters one row expanded to [b, 8], dt a float, and the evaluation may be replayed from a HIP
    # graph (``_maybe_graph``).  Several: every sample carries its own timestep image (``t_img`` [b, 512]), SE(3) step parameters
    # and step size (s2s_se3_step dt_per_sample), gathered by its row ``idx`` of the concatenated tables; never captured.
    per_sample = len(groups) > 1
    timg, p8s, base, o = [], [], {}, 0
    for k in order:
        t_all = torch.as_tensor(np.ascontiguousarray(groups[k]["ts"], dtype=np.float64)).float()   # fl32(t), as `t * torch.ones(B)` gives
        p8s.append(diffuser.step_params(t_all).to(device))   # [n_k, 8]: t is uniform over the group
        # timestep embeddings of the whole schedule, uploaded once (same host function the network would call per step), and their
        # first-layer images (the embedder's only t-dependent arithmetic) for the whole schedule at once
        timg.append(emb.time_images(emb.time_embed(t_all).to(device)))
        base[k] = o
        o += len(t_all)
    TIMG, P8 = (torch.cat(timg).contiguous(), torch.cat(p8s).contiguous()) if per_sample else (timg[0], p8s[0])
    defer_psi = trace is None   # the psi blend is deferred to the last evaluation unless the steps are recorded

    def eager(f):
        return _net_eval(net, f, defer_psi)

    with _backbone_deferred(net):
        rig = sc = idx = dtv = feats = mask = diffuse_mask = graphed = None
        members, run = [], eager
        for g in range(n_max):
            joining = [k for k in order if n_max - len(groups[k]["ts"]) == g]
            for k in joining:
                rk = groups[k]["rigids_t"]
                bk = rk.shape[0]
                fk = dict(groups[k]["feats"])
                # the masks as float32 device tensors ONCE per batch composition: the network's per-chunk caches (embedder terms, mask
                # terms) key on their identity
                for m in ("residue_mask", "fixed_mask"):
                    fk[m] = fk[m].to(device).float().contiguous()
                # ("t" is not read: every sample's timestep enters through its t_img row)
                fk.update(rigids_t=rk, sc_ca_t=torch.zeros(bk, N, 3, device=device), t=torch.zeros(bk), t_img=TIMG[base[k]])
                if not per_sample:
                    graphed = _maybe_graph(net, fk, bk, N, trace, n_max)
                    run = graphed if graphed is not None else eager
                sck = fk["sc_ca_t"]
                if self_conditioning:      # the group's extra evaluation at its first t with an empty self-conditioning input, on its own
                    sck = run(fk)["rigids7"][..., 4:].clone()
                rig = rk if rig is None else torch.cat([rig, rk])
                sc = sck if sc is None else torch.cat([sc, sck])
                if per_sample:
                    ik = torch.full((bk,), base[k], dtype=torch.int64, device=device)
                    dk = torch.full((bk,), float(groups[k]["dt"]), dtype=torch.float64, device=device)
                    idx = ik if idx is None else torch.cat([idx, ik])
                    dtv = dk if dtv is None else torch.cat([dtv, dk])
                members.append((k, bk, fk))
            b = rig.shape[0]
            if joining:
                if len(members) == 1:
                    feats = members[0][2]      # the very tensors of the group's own evaluation: the network's caches stay valid
                else:
                    feats = {key: torch.cat([f[key].to(device) for _, _, f in members]) for key in _REPEAT_KEYS if key in members[0][2]}
                    feats["t"] = torch.zeros(b)
                mask = feats["residue_mask"]
                diffuse_mask = ((1 - feats["fixed_mask"]) * mask).contiguous()
            feats["rigids_t"], feats["sc_ca_t"] = rig, sc
            feats["t_img"] = TIMG.index_select(0, idx) if per_sample else TIMG[g]
            out = run(feats)
            x0_7 = out["rigids7"]
            t = float(groups[order[0]]["ts"][g])     # (trace: the longest trajectory's t)
            if g == n_max - 1:           # every trajectory's last evaluation (t == min_t): the x0 prediction is the sample
                if trace is not None:
                    trace.append(dict(t=t, rigids_t=rig, sc_ca_t=sc, x0=x0_7, psi=out["psi"]))
                break
            sc_in = sc
            if self_conditioning:
                sc = x0_7[..., 4:].clone() if graphed is not None else x0_7[..., 4:]   # (a replay overwrites the static output)
            z = host_noise() if host_noise is not None else None
            z_rot, z_trans = z if z is not None else (None, None)
            if not probability_flow and z_rot is None:
                z_rot = torch.randn(b, N, 3, dtype=torch.float64, device=device)
                z_trans = torch.randn(b, N, 3, dtype=torch.float64, device=device)
            p8, dt = (P8.index_select(0, idx), dtv) if per_sample else (P8[g].expand(b, 8).contiguous(), groups[0]["dt"])
            nxt, rs, tsc = diffuser.step(x0_7, rig, p8, dt, mask, diffuse_mask, center_trans=center_mode, noise_scale=noise_scale,
                                         probability_flow=probability_flow, z_rot=z_rot, z_trans=z_trans, want_scores=trace is not None)
            if trace is not None:
                trace.append(dict(t=t, rigids_t=rig, sc_ca_t=sc_in, x0=x0_7, psi=out["psi"], rot_score=rs, trans_score=tsc, next7=nxt))
            rig = nxt
            if per_sample:
                idx = idx + 1
        psi = out["psi"]
        if out.get("psi_deferred"):   # the blend with the input torsion under the fixed mask, once (DenoisingNet.blend_psi)
            psi = net.blend_psi(psi, feats["torsion_angles_sin_cos"], feats["fixed_mask"])
        atom37 = compute_backbone(out["rigids"], psi, aatype=feats.get("aatype"), _rigids7=x0_7)[0]
    samples, o = [None] * len(groups), 0
    for k, bk, _ in members:
        samples[k] = (atom37[o:o + bk], x0_7[o:o + bk], psi[o:o + bk])
        o += bk
    return samples, x0_7


def _require_hip_device(device, net) -> torch.device:
    device = torch.device(device) if device is not None else next(net.parameters()).device
    if device.type != "cuda":
        raise ops.HipLibraryError("the sampler needs the HIP device (MI355X); there is no CPU fallback")
    return device


def _start_frames(diffuser, batch: dict, rigids_0: Rigid, t_delta: float, lo: int, hi: int, rng: str, device):
    """The noised frames a chunk's trajectory starts from, for the replicas [lo, hi) of the chunk ``rigids_0`` -> [hi - lo, N, 7]
    float32 device tensor, or None for an empty slice.  ``rng="host"``: drawn once per trajectory on the host generators for the
    WHOLE chunk, in the reference's order (diffusion_module.py:277-296 there) -- also for an empty slice; ``rng="device"``
    (throughput mode): for the slice only, drawn and applied on the device (s2s_forward_marginal)."""
    B_total, N = rigids_0.shape[0], rigids_0.shape[1]
    b = hi - lo
    if rng == "device":
        if b == 0:
            return None
        if t_delta > 0:
            dmask = batch["residue_mask"].to(device).float().reshape(1, N).expand(b, N).contiguous()
            return diffuser.forward_marginal_device(rigids_0[lo:hi].to_tensor_4x4().to(device), t_delta, dmask)
        return diffuser.forward_marginal_device(None, None, shape=(b, N))
    # ~300 small host tensor operations on [B, N, 3..9] values: with every core of the host in torch's intra-op pool each of them pays
    # the pool's wake-up (tens of ms per chunk on a 128-thread box, in front of the GPU work); element-wise arithmetic and reductions
    # over the last axis do not depend on the thread count, so the frames are the same bits.  S2S_HOST_FM_THREADS=0: leave the pool alone.
    nt, keep = int(os.environ.get("S2S_HOST_FM_THREADS", "1")), torch.get_num_threads()
    if nt > 0 and nt != keep:
        torch.set_num_threads(nt)
    try:
        if t_delta > 0:
            rigids_t = diffuser.forward_marginal(rigids_0=rigids_0.to(device="cpu"), t=t_delta * torch.ones(B_total),
                                                 diffuse_mask=batch["residue_mask"].cpu().repeat(B_total, 1),
                                                 as_tensor_7=True)["rigids_t"]
        else:
            rigids_t = diffuser.sample_prior(shape=rigids_0.shape, device="cpu", as_tensor_7=True)["rigids_t"]
    finally:
        if nt > 0 and nt != keep:
            torch.set_num_threads(keep)
    if b == 0:
        return None
    return rigids_t[lo:hi].to(device).float().contiguous()


def _burn_step_draws(B_total: int, N: int, n_draw_steps: int):
    """The reference consumes two float64 normal draws of the whole chunk per step even under the probability-flow ODE
    (so3.py:360, r3.py:109): consume them so that the host generator is where the reference's is for the next chunk.  Nothing reads the
    values, so the generator is fast-forwarded over them where that is exact (ops.host_rng_discard_float64_normals: the engine's
    position after the draws, checked against real draws once per process); otherwise they are drawn."""
    if ops.host_rng_discard_float64_normals(B_total * N * 3, 2 * n_draw_steps):
        return
    for _ in range(n_draw_steps):
        torch.randn(B_total, N, 3, dtype=torch.float64)
        torch.randn(B_total, N, 3, dtype=torch.float64)


def _skips_unused_draws(probability_flow: bool, B_total: int, N: int) -> bool:
    """Under the probability-flow ODE the reference's per-step draws are consumed, not used.  Where the host generator can be
    fast-forwarded over them (``_burn_step_draws``: milliseconds per chunk) that happens right behind the chunk's start frames;
    otherwise they are drawn step by step inside the loop, behind the GPU work (``_sample_batch.host_noise``)."""
    return probability_flow and ops.host_rng_can_discard(B_total * N * 3)


def _chunk_rigids(gt_frames_4x4: torch.Tensor, bsz: int) -> Rigid:
    """The ground-truth frames of one target [1, N, 4, 4] as a chunk of ``bsz`` replicas."""
    return Rigid.from_tensor_4x4(gt_frames_4x4.repeat(bsz, *(1,) * (gt_frames_4x4.ndim - 1)))


def _expand_features(batch: dict, b: int, device) -> dict:
    """The per-sample features of one target (batch dimension 1) for ``b`` replicas, on the device."""
    return {k: batch[k].to(device).repeat(b, *(1,) * (batch[k].ndim - 1)) for k in _REPEAT_KEYS if k in batch}


def _draw_entries(diffuser, batch: dict, rig0, N: int, scheds, entries, *, rng: str, probability_flow: bool, device):
    """THE walk over the host noise stream for one batch.  ``entries`` = [(i, chunk_size, lo, hi)]: consecutive (t_delta ``scheds[i]``
    = (t_delta, n, dt, ts), replica chunk) entries of the reference's stream (t_delta-major, chunk-minor; diffusion_module.py:341-367),
    (lo, hi) = this rank's slice of the chunk; ``rig0(chunk_size)`` = the chunk's ground-truth frames.  Per entry, in order: the WHOLE
    chunk's start frames (``rng="host"``: also for an empty slice -- every generator stays in lock-step with the other ranks;
    ``rng="device"``: an empty slice draws nothing, the host generator is never touched), then the two float64 draws per step of its
    n - 1 steps -- burnt right behind the start frames, because the next entry's start frames come after them.  Only the LAST entry's
    may be deferred: they ride in the loop, behind the GPU work, when its trajectory is the longest of the batch (so one draw pair goes
    per global step from step 0) and the generator cannot be fast-forwarded over them (``_skips_unused_draws``; under the SDE they are
    used, so never).  -> ({i: [start frames of the non-empty slices]}, deferred entry (chunk_size, lo, hi, steps) or None)."""
    n_max = max(scheds[i][1] for i, _, _, _ in entries)
    starts, tail = {}, None
    for e, (i, bsz, lo, hi) in enumerate(entries):
        if hi == lo and rng == "device":
            continue
        t_delta, n = scheds[i][:2]
        r = _start_frames(diffuser, batch, rig0(bsz), t_delta, lo, hi, rng, device)
        if rng == "host":
            if e + 1 == len(entries) and n == n_max and not _skips_unused_draws(probability_flow, bsz, N):
                tail = (bsz, lo, hi, n - 1)     # drawn for real: rides in the loop, behind the GPU (global step == its local step)
            else:
                _burn_step_draws(bsz, N, n - 1)
        if r is not None:
            starts.setdefault(i, []).append(r)
    if not starts and tail is not None:     # nothing to sample on this rank: nothing reads the draws, the generator goes past them
        _burn_step_draws(tail[0], N, tail[3])
    return starts, tail


@torch.no_grad()
def _sample_batch(net, diffuser, batch: dict, rig0, N: int, scheds, entries, *, noise_scale: float, probability_flow: bool,
                  self_conditioning: bool, device, rng: str, trace: Optional[list] = None) -> dict:
    """One batch of the plan (``entries``, see ``_draw_entries``): its draws, then ONE guarded pass over one group of samples per
    t_delta -> {i: (atom37, rigids7, psi)} for the t_deltas of the batch, this rank's replicas in replica order ({} when it has none)."""
    starts, tail = _draw_entries(diffuser, batch, rig0, N, scheds, entries, rng=rng, probability_flow=probability_flow, device=device)
    if not starts:
        return {}

    bsz, lo, hi = tail[:3] if tail is not None else (0, 0, 0)

    def host_noise():
        # the reference consumes two float64 normal draws of the whole chunk per step even under the probability-flow ODE
        # (so3.py:360, r3.py:109): keep the host generator in lock-step for later chunks; the SDE uses this rank's slice of them
        zr = torch.randn(bsz, N, 3, dtype=torch.float64)
        zt = torch.randn(bsz, N, 3, dtype=torch.float64)
        if probability_flow:
            return None
        return zr[lo:hi].to(device).contiguous(), zt[lo:hi].to(device).contiguous()

    groups = []
    for i, rs in starts.items():
        rigids_t = torch.cat(rs, dim=0) if len(rs) > 1 else rs[0]
        groups.append(dict(rigids_t=rigids_t, ts=scheds[i][3], dt=scheds[i][2], feats=_expand_features(batch, rigids_t.shape[0], device)))
    samples = _guarded_pass(net, diffuser, groups, noise_scale=noise_scale, probability_flow=probability_flow,
                            self_conditioning=self_conditioning, center_mode=1, host_noise=host_noise if tail is not None else None,
                            trace=trace)
    return dict(zip(starts, samples))


def forward_backward(net, diffuser, batch: dict, rigids_0: Rigid, t_delta: float, *, num_timesteps: int,
                     min_t: float = 0.01, noise_scale: float = 1.0, probability_flow: bool = True,
                     self_conditioning: bool = True, device=None, shard: Tuple[int, int] = (0, 1),
                     replica_slice: Optional[Tuple[int, int]] = None, rng: str = "host", trace: Optional[list] = None,
                     return_rigids: bool = False):
    """-> atom37 [b, N, 37, 3] float32 DEVICE tensor for this rank's replica slice (b = hi - lo).

    The chunk (``rigids_0.shape[0]`` replicas) is the unit of the reference's host noise stream.  ``replica_slice`` =
    (lo, hi) selects the replicas of the chunk THIS process samples (``shard`` = (rank, world) is the ceil split of
    the chunk); in ``rng="host"`` mode every process still draws the whole chunk's noise in the reference's order --
    including a process whose slice is empty -- so the union over processes equals the single-process run sample for
    sample and every generator stays in lock-step for later chunks.  ``rng="device"`` (throughput mode) draws the
    forward-marginal and step noise on the device generator for the slice only."""
    device = _require_hip_device(device, net)
    B_total, N = rigids_0.shape[0], rigids_0.shape[1]
    lo, hi = replica_slice if replica_slice is not None else shard_range(B_total, *shard)
    if not (0 <= lo <= hi <= B_total):
        raise ValueError(f"replica_slice {(lo, hi)} outside the chunk of {B_total} replicas")
    T, n, dt, ts = schedule(t_delta, num_timesteps, min_t)
    out = _sample_batch(net, diffuser, batch, lambda bsz: rigids_0, N, [(t_delta, n, dt, ts)], [(0, B_total, lo, hi)],
                        noise_scale=noise_scale, probability_flow=probability_flow, self_conditioning=self_conditioning, device=device,
                        rng=rng, trace=trace)
    if not out:
        return torch.zeros(0, N, 37, 3, device=device)
    return out[0] if return_rigids else out[0][0]


_MERGE_MAX_PAIRS = 8 << 20   # a merged trajectory stays within the working set of BASELINE configs[1] (128 x 256^2 pairs, ~11 GB)


def merge_chunk_groups(chunks, N: int, *, mergeable: bool = True, max_pairs: int = None):
    """Consecutive replica chunks ``[(chunk_size, lo, hi)]`` (``rank_chunk_slices``) -> groups that are sampled as ONE trajectory each.
    A group grows while this rank's replicas in it stay below ``max_pairs`` pairs; ``S2S_MERGE_CHUNKS=0`` (or ``mergeable=False``:
    host noise under the SDE, where a chunk's per-step draws interleave with its trajectory) keeps one chunk per group."""
    max_pairs = _MERGE_MAX_PAIRS if max_pairs is None else max_pairs
    if not mergeable or os.environ.get("S2S_MERGE_CHUNKS", "1") == "0":
        return [[c] for c in chunks]
    groups, cur, cur_b = [], [], 0
    for c in chunks:
        b = c[2] - c[1]
        if cur and (cur_b + b) * N * N > max_pairs:
            groups.append(cur)
            cur, cur_b = [], 0
        cur.append(c)
        cur_b += b
    if cur:
        groups.append(cur)
    return groups


def merge_delta_groups(steps, b: int, N: int, max_pairs: int = None):
    """Consecutive t_deltas (``steps[i]`` = their trajectory lengths) -> groups [[i, ...]] sampled as one growing batch each: a group
    holds at most ``max_pairs`` pairs at its end (b replicas per t_delta).  ``S2S_MERGE_DELTAS=0``: one t_delta per group."""
    max_pairs = _MERGE_MAX_PAIRS if max_pairs is None else max_pairs
    per = max(1, b) * N * N
    cap = 1 if os.environ.get("S2S_MERGE_DELTAS", "1") == "0" else max(1, max_pairs // per)
    return [list(range(i, min(i + cap, len(steps)))) for i in range(0, len(steps), cap)]


def _batch_plan(chunks, steps, N: int, *, merge_deltas: bool, merge_chunks: bool, max_pairs: int = None):
    """The flat plan of a target: the stream of (t_delta i, chunk) entries, t_delta-major, cut into batches of consecutive entries ->
    [(t_deltas [i, ...] that are complete after these batches, [entries [(i, chunk_size, lo, hi)] per batch])].  Several t_deltas
    whose replicas fit the pair budget are ONE batch (``merge_delta_groups``); otherwise the chunks of a t_delta that fit it are
    (``merge_chunk_groups``; ``merge_chunks=False``: one entry per batch)."""
    b_rank = sum(hi - lo for _, lo, hi in chunks)
    plan = []
    for grp in (merge_delta_groups(steps, b_rank, N, max_pairs) if merge_deltas else [[i] for i in range(len(steps))]):
        if len(grp) > 1:
            plan.append((grp, [[(i, *c) for i in grp for c in chunks]]))
        else:
            plan.append((grp, [[(grp[0], *c) for c in cg] for cg in merge_chunk_groups(chunks, N, mergeable=merge_chunks, max_pairs=max_pairs)]))
    return plan


def forward_backward_chunks(net, diffuser, batch: dict, gt_frames_4x4: torch.Tensor, chunks, t_delta: float, *, num_timesteps: int,
                            min_t: float = 0.01, noise_scale: float = 1.0, probability_flow: bool = True,
                            self_conditioning: bool = True, device=None, rng: str = "host", max_pairs: int = None):
    """All replica chunks of one (target, t_delta) -> atom37 [sum(hi - lo), N, 37, 3] in replica order (``forward_backward_deltas``
    of one t_delta).

    The reference samples ``n_replica`` replicas in chunks of ``replica_per_batch`` (diffusion_module.py:341-351), one trajectory per
    chunk; its default block (100 replicas in chunks of 64 + 36 on chains of 35 .. 80 residues) leaves the GPU launch-bound -- an
    evaluation of 64 x 35^2 pairs costs what one of 100 x 35^2 costs.  The chunk is only the unit of the reference's HOST NOISE
    stream: every replica's trajectory is independent of its batch (the kernels are batch-invariant: sharded == single is tested
    bit for bit).  So the chunks' start frames are drawn chunk by chunk in the reference's order (and, in ``rng="host"`` mode, the
    two float64 draws per step the reference consumes even under the ODE are consumed per chunk), and the chunks that fit a pair
    budget run as ONE trajectory: same samples, file for file, in fewer launches.  Under the SDE with host noise the per-step draws
    are part of the trajectory: one chunk per trajectory, as before.  ``chunks`` = ``rank_chunk_slices(...)`` of this rank."""
    return forward_backward_deltas(net, diffuser, batch, gt_frames_4x4, chunks, [t_delta], num_timesteps=num_timesteps, min_t=min_t,
                                   noise_scale=noise_scale, probability_flow=probability_flow, self_conditioning=self_conditioning,
                                   device=device, rng=rng, max_pairs=max_pairs)[0]


def forward_backward_deltas(net, diffuser, batch: dict, gt_frames_4x4: torch.Tensor, chunks, delta_range, **kw):
    """``iter_forward_backward_deltas`` collected: [atom37 [sum(hi - lo), N, 37, 3] per t_delta] in ``delta_range`` order."""
    delta_range = list(delta_range)
    out = [None] * len(delta_range)
    for idx, a37s in iter_forward_backward_deltas(net, diffuser, batch, gt_frames_4x4, chunks, delta_range, **kw):
        for i, a in zip(idx, a37s):
            out[i] = a
    return out


def iter_forward_backward_deltas(net, diffuser, batch: dict, gt_frames_4x4: torch.Tensor, chunks, delta_range, *, num_timesteps: int,
                                 min_t: float = 0.01, noise_scale: float = 1.0, probability_flow: bool = True,
                                 self_conditioning: bool = True, device=None, rng: str = "host", max_pairs: int = None):
    """All t_deltas of one target (the outer loop of the reference's predict_step, diffusion_module.py:341-367) -> per group of
    t_deltas (indices [i, ...] into ``delta_range``, [atom37 [sum(hi - lo), N, 37, 3] per t_delta]), as soon as the group is sampled.

    The reference's default block runs 10 t_deltas (0.25 .. 0.70 of 1000 timesteps: trajectories of 250 .. 700 steps) of 100 replicas
    one after the other; on chains of 35 .. 80 residues every network evaluation is then bound by the latency of its ~83 dependent
    launches, not by the GPU.  A replica's trajectory does not depend on its batch, and nothing in the network or in the SE(3) step
    couples the samples of a batch -- so the t_deltas whose replicas fit the pair budget run as ONE batch that GROWS: aligned at
    their common end (t = min_t), the longest trajectory starts alone and each shorter one joins when as many steps remain as it
    has, with its own timestep image, step parameters and step size per sample (``_denoise_pass``).  4750 + 10 evaluations of
    100 replicas become 700 + 10 of 100 .. 1000.  The host noise stream keeps the reference's order: start frames t_delta by t_delta,
    chunk by chunk, each chunk's (unused, under the ODE) per-step draws consumed before the next chunk's start frames -- the last
    chunk's ride in the loop when its trajectory is the longest (``_draw_entries``).  Under the SDE the per-step draws are part of a
    trajectory (host noise: in the reference's order; device noise: a merged batch would draw them for the growing batch, i.e. other
    samples than one t_delta at a time under the same seed): one t_delta at a time, as the reference does."""
    device = _require_hip_device(device, net)
    N = gt_frames_4x4.shape[-3]
    scheds = [(float(t),) + schedule(float(t), num_timesteps, min_t)[1:] for t in delta_range]    # (t_delta, n, dt, ts)
    merge_deltas = probability_flow and len(scheds) > 1 and sum(hi - lo for _, lo, hi in chunks) > 0 and all(s[0] > 0 for s in scheds) \
        and hasattr(getattr(net, "embedder", None), "time_images")
    plan = _batch_plan(chunks, [s[1] for s in scheds], N, merge_deltas=merge_deltas, merge_chunks=probability_flow or rng == "device",
                       max_pairs=max_pairs)
    for grp, batches in plan:
        pieces = {i: [] for i in grp}
        for entries in batches:   # (never yield inside torch.no_grad() -- ``_sample_batch`` -- the caller would inherit the grad mode)
            done = _sample_batch(net, diffuser, batch, lambda bsz: _chunk_rigids(gt_frames_4x4, bsz), N, scheds, entries,
                                 noise_scale=noise_scale, probability_flow=probability_flow, self_conditioning=self_conditioning,
                                 device=device, rng=rng)
            for i, sample in done.items():
                pieces[i].append(sample[0])
        yield grp, [(torch.cat(p, dim=0) if len(p) > 1 else p[0]) if p else torch.zeros(0, N, 37, 3, device=device) for p in pieces.values()]


def forward_flops(n_res: int) -> float:
    """Algorithmic FLOPs of one network evaluation per replica: F(N) = 2,251,264 N^2 + 3.24e7 N."""
    return 2251264.0 * n_res * n_res + 3.24e7 * n_res


def plan_mixed_work(lengths, replicas: int, world: int = 1, *, max_pairs: int = 24 << 20, ms_per_mpair: float = 10.7,
                    launch_floor_ms: float = 4.0):
    """Work distribution for many chains of different length (BASELINE configs[4]): flatten to (chain,
    replica block) items, balance them over the ranks by FLOP weight, bucket each rank's items by padded length.

      1. every chain's replicas are ceil-split into ``world`` blocks (``shard_range``); the non-empty blocks are the items,
         weight = (replicas in the block) x F(N);
      2. longest-processing-time-first: items in decreasing weight go to the currently least loaded rank (even splits give
         every rank the same set of lengths; remainders and replicas < world are what the weights are for);
      3. per rank, items in decreasing length are packed into padded batches (n_pad = the longest chain of the batch; the
         kernels take ragged N, so there is no tile rounding).  An item joins the open batch when that is cheaper than a
         batch of its own (within 5 %) under  cost(batch) = max(launch_floor_ms, ms_per_mpair x padded Mpairs)  per network evaluation
         -- one evaluation is ~83 dependent launches, so small batches are launch-bound and padding them into a neighbour is free,
         while large ones pay for every padded pair (measured: 10.7 ms per 2^20 pairs at cfg2) -- and the batch stays
         below ``max_pairs`` (device memory: ~1.3 KB per pair).
    -> plan[rank] = [ {"n_pad": int, "items": [(chain, replica_lo, replica_hi), ...]}, ... ]"""
    lengths = [int(x) for x in lengths]
    items = []
    for k, L in enumerate(lengths):
        for r in range(world):
            lo, hi = shard_range(replicas, r, world)
            if hi > lo:
                items.append((forward_flops(L) * (hi - lo), k, lo, hi))
    items.sort(key=lambda it: (-it[0], it[1], it[2]))
    load = [0.0] * world
    mine = [[] for _ in range(world)]
    for w, k, lo, hi in items:
        r = min(range(world), key=lambda q: (load[q], q))
        load[r] += w
        mine[r].append((k, lo, hi))
    plan = []
    for r in range(world):
        cost = lambda pairs: max(launch_floor_ms, ms_per_mpair * pairs / float(1 << 20))  # noqa: E731
        batches, cur, cur_b, n_pad = [], [], 0, 0
        for k, lo, hi in sorted(mine[r], key=lambda it: (-lengths[it[0]], it[0], it[1])):
            L, b = lengths[k], hi - lo
            if cur:
                merged = (cur_b + b) * n_pad * n_pad
                if merged > max_pairs or cost(merged) > 1.05 * (cost(cur_b * n_pad * n_pad) + cost(b * L * L)):
                    batches.append({"n_pad": n_pad, "items": cur})
                    cur, cur_b = [], 0
            if not cur:
                n_pad = L
            cur.append((k, lo, hi)); cur_b += b
        if cur:
            batches.append({"n_pad": n_pad, "items": cur})
        plan.append(batches)
    return plan


def mixed_batch_seed(base_seed: int, t_delta: float, chain: int, replica_lo: int) -> int:
    """Seed of the host generators for the padded batch whose first item is (chain, replica_lo): a function of the run seed and the
    work item only, so no two batches of a run -- on one rank or on different ranks -- share a noise stream."""
    return (int(base_seed) * 1000003 + int(round(float(t_delta) * 1000)) * 998244353 + int(chain) * 7919 + int(replica_lo) * 104729
            + 12345) % (2 ** 63 - 1)


@torch.no_grad()
def sample_mixed_lengths(net, diffuser, targets, replicas: int, t_delta: float, *, num_timesteps: int,
                         min_t: float = 0.01, noise_scale: float = 1.0, probability_flow: bool = True,
                         self_conditioning: bool = True, device=None, rigids_t_init=None, shard: Tuple[int, int] = (0, 1),
                         rng: str = "host", max_pairs: int = 24 << 20, plan=None, seed_base: Optional[int] = None):
    """BASELINE configs[4]: many chains of different length, ``replicas`` each, in padded batches.

    The reference cannot do this (`assert batch size == 1`, diffusion_module.py:249) and its padding semantics
    would be wrong for it (float key-padding mask added to the transformer logits, centre of mass over padded
    residues).  Here padding is exact: padded keys are removed from both attentions, pair rows/cols are
    masked, the centre of mass runs over real residues only -- so every chain reproduces its own un-padded run.
    Work is distributed by ``plan_mixed_work`` (FLOP-weighted over ``shard`` = (rank, world), bucketed by length).
    ``targets``: list of single-target feature dicts (batch dim 1).  ``rng="device"`` draws the forward-marginal / step
    noise on the device; "host" on the host generator per (chain, block) in plan order; ``rigids_t_init[k]`` [replicas,
    N_k, 7] overrides the starting frames.
    -> list over chains of (replica_lo, atom37 [b, N_k, 37, 3]) pieces this rank sampled, in replica order."""
    device = torch.device(device) if device is not None else next(net.parameters()).device
    lengths = [int(t["aatype"].shape[1]) for t in targets]
    rank, world = shard
    if plan is None:
        plan = plan_mixed_work(lengths, replicas, world, max_pairs=max_pairs)
    T, n, dt, ts = schedule(t_delta, num_timesteps, min_t)
    pieces = [[] for _ in targets]
    tr = net.translator
    keep = tr.exact_padding
    tr.exact_padding = True
    base_seed = int(torch.initial_seed()) if seed_base is None else int(seed_base)
    # The per-batch seeding below re-seeds the process-global host generators; their states are put back on the way out, so that the
    # call leaves no trace in them: `torch.initial_seed()` stays the run seed for the next call (a loop over t_delta without
    # ``seed_base`` sees the same base every time) and whatever the caller samples afterwards continues ITS stream.
    host_states = (torch.get_rng_state(), np.random.get_state()) if rng == "host" else None
    try:
        for batch in plan[rank]:
            n_pad = batch["n_pad"]
            if rng == "host":
                # The host generators are seeded per batch from (run seed, t_delta, first (chain, replica) item of the batch): every
                # rank starts from the same run seed (eval.py), and without this each rank would draw the noise of ITS blocks from the
                # same stream -- identical starting frames and step noise for replica blocks 0-24, 25-49, ... of a chain, i.e. duplicate
                # conformations in the gathered ensemble.  (The device mode offsets its Philox seed by the rank instead.)
                ti0, lo0, _ = batch["items"][0]
                item_seed = mixed_batch_seed(base_seed, t_delta, ti0, lo0)
                torch.random.default_generator.manual_seed(item_seed)   # the CPU generator only: the device stream is not touched
                np.random.seed(item_seed % (2 ** 32))
            rows, r_t = {k: [] for k in _REPEAT_KEYS}, []
            for ti, lo, hi in batch["items"]:
                tg, L, b = targets[ti], lengths[ti], hi - lo
                for k in _REPEAT_KEYS:
                    v = tg[k]
                    pad = torch.zeros((1, n_pad - L) + tuple(v.shape[2:]), dtype=v.dtype)
                    if k == "residue_idx" and L < n_pad:  # keep padded indices inside the real range (table lookups stay in bounds)
                        pad = pad + v[:, -1:]
                    rows[k].append(torch.cat([v.cpu(), pad], dim=1).repeat(b, *(1,) * (v.ndim - 1)))
                gt4 = tg["rigidgroups_gt_frames"][..., 0, :, :]
                if rigids_t_init is not None:
                    rt = rigids_t_init[ti][lo:hi].to(device).float()
                else:   # the block is its own chunk of the noise stream (no step draws: the ODE's are not consumed here)
                    rt = _start_frames(diffuser, tg, _chunk_rigids(gt4, b), t_delta, 0, b, rng, device)
                ident = torch.zeros(b, n_pad - L, 7, device=device)
                ident[..., 0] = 1.0  # identity frames on the padding: finite everywhere, masked out of every result
                r_t.append(torch.cat([rt, ident], dim=1))
            feats = {k: torch.cat(v, dim=0).to(device) for k, v in rows.items()}
            rigids_t = torch.cat(r_t, dim=0).contiguous()
            atom37, _, _ = denoise_loop(net, diffuser, feats, rigids_t, ts, dt, min_t=min_t, noise_scale=noise_scale,
                                        probability_flow=probability_flow, self_conditioning=self_conditioning, center_mode=2)
            o = 0
            for ti, lo, hi in batch["items"]:
                pieces[ti].append((lo, atom37[o:o + hi - lo, :lengths[ti]].clone()))
                o += hi - lo
    finally:
        tr.exact_padding = keep
        if host_states is not None:
            torch.set_rng_state(host_states[0])
            np.random.set_state(host_states[1])
    return [sorted(p, key=lambda x: x[0]) for p in pieces]
