"""Python binding of libstr2str_hip.so (include/str2str_hip.h) over ctypes.

torch is plumbing here: it owns device memory and the current HIP stream; every op below hands raw
device pointers + sizes + the stream to one C-ABI entry point.  There is NO fallback: if the
library is missing or a tensor is not a contiguous float32 CUDA(HIP) tensor the op raises.
The ops are also registered as ``torch.ops.str2str_amd.*`` custom ops (``register_torch_ops``).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STR2STR_HIP_LIB") or os.path.join(_HERE, "libstr2str_hip.so")  # env override: A/B builds
ABI_VERSION = 34

_lib = None
_tables_loaded = set()   # device indices that hold the backbone tables

_vp, _i, _f, _d, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong

_SIGNATURES = {
    "s2s_abi_version": [],
    "s2s_edge_transition": [_vp] * 12 + [_i, _i, _f, _vp, _vp, _vp, _vp, _vp],
    "s2s_edge_transition_f16x3": [_vp] * 9 + [_i, _i, _f, _i, _vp, _vp, _vp, _i, _vp, _vp],
    "s2s_edge_embed": [_vp] * 15 + [_i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp],
    "s2s_edge_embed_f16x3": [_vp] * 14 + [_i, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp],
    "s2s_pair_project": [_vp] * 5 + [_i, _i, _vp],
    "s2s_ipa_prep_points": [_vp] * 6 + [_ll, _i, _i, _i, _i, _vp],
    "s2s_ipa_attention": [_vp] * 12 + [_i, _i, _i, _i, _i, _i, _i, _f, _f, _vp],
    "s2s_ipa_opair": [_vp] * 4 + [_i, _i, _i, _i, _i, _i, _i, _vp],
    "s2s_ipa_prep_points_f16": [_vp] * 9 + [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "s2s_ipa_attention_f16w": [_vp] * 15 + [_i] * 8 + [_f, _f, _i, _vp],
    "s2s_rigid_compose_update": [_vp] * 4 + [_ll, _i, _vp],
    "s2s_torsion_head": [_vp, _i, _i, _vp, _ll, _vp, _f, _vp, _ll, _vp],
    "s2s_rigid_scale_trans": [_vp, _vp, _ll, _f, _i, _vp],
    "s2s_set_backbone_tables": [_vp] * 4,
    "s2s_frames_to_backbone": [_vp] * 5 + [_ll, _vp],
    "s2s_se3_step": [_vp] * 12 + [_i, _i, _d, _vp, _d, _i, _i, _d, _vp],
    "s2s_forward_marginal": [_vp] * 7 + [_i, _vp, _vp, _f, _vp, _i, _i, _vp],
    "s2s_pack_planes": [_vp, _ll, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp],
    "s2s_node_linear": [_vp, _vp, _vp, _ll, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp],
    "s2s_node_linear_f32": [_vp, _i, _vp, _vp, _ll, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _i, _i, _vp],
    "s2s_node_linear_multi": [_vp, _i, _vp, _vp],
    "s2s_node_chain": [_vp, _vp, _i, _ll, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _f, _vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp],
    "s2s_embed_assemble": [_vp, _ll, _vp, _ll, _vp, _vp, _ll, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp],
    "s2s_row_layernorm": [_vp, _i, _ll, _i, _vp, _vp, _f, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp],
    "s2s_node_linear_vfrag": [_vp, _vp, _vp, _ll, _i, _i, _i, _vp, _i, _i, _vp, _vp],
    "s2s_encoder_attention": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "s2s_encoder_attention_f16x3": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "s2s_ca_sample_stats": [_vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp],
    "s2s_ca_pairwise_distances": [_vp, _i, _i, _i, _vp, _vp],
    "s2s_ca_pwd_js": [_vp, _i, _vp, _i, _i, _i, _i, _d, _vp, _vp, _vp, _vp],
    "s2s_ca_rmsd_matrix": [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _ll, _vp],
    "s2s_ca_superpose": [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp],
    "s2s_apply_xform": [_vp, _vp, _i, _ll, _vp, _vp],
    "s2s_format_pdb_models": [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _ll],
    "s2s_write_pdb_models": [ctypes.c_char_p, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i],
    "s2s_merge_pdb_files": [_vp, _i, ctypes.c_char_p],
    "s2s_mt19937_discard": [_vp, _vp, _vp, ctypes.c_ulonglong],
}
_LL_RETURN = ("s2s_format_pdb_models", "s2s_write_pdb_models", "s2s_merge_pdb_files")
EXPORTS = tuple(_SIGNATURES)


class HipLibraryError(RuntimeError):
    pass


class WeightRangeError(HipLibraryError):
    """A weight does not fit the f16x3 packing (|32 w| >= 65504)."""


class KernelTimer:
    """Optional per-launch timing with HIP events recorded on the launch stream (bench.py's
    ``roofline`` leg).  ``with KernelTimer("s2s_edge_transition") as kt: ...; kt.mean_ms()``."""

    active = None

    def __init__(self, *names):
        self.names = set(names)
        self.events = {n: [] for n in names}
        self.work = {n: [0, 0] for n in names}   # algorithmic [flops, bytes] of the timed launches, where the wrapper states them

    def __enter__(self):
        KernelTimer.active = self if self.names else None   # no names: a no-op context (HIP graphs stay enabled)
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None

    def mean_ms(self, name):
        torch.cuda.synchronize()
        ev = self.events[name]
        return (sum(a.elapsed_time(b) for a, b in ev) / len(ev)) if ev else float("nan"), len(ev)

    def total_ms(self, name):
        torch.cuda.synchronize()
        ev = self.events[name]
        return sum(a.elapsed_time(b) for a, b in ev), len(ev)


def _timed(name, launch, flops=0, nbytes=0):
    kt = KernelTimer.active
    if kt is None or name not in kt.names:
        return launch()
    kt.work[name][0] += int(flops)
    kt.work[name][1] += int(nbytes)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = launch()
    b.record()
    kt.events[name].append((a, b))
    return rc


def load_library(path: Optional[str] = None):
    """dlopen the kernel library and type its entry points (no GPU needed for this)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise HipLibraryError(
            f"{p} not found: the HIP kernels are not built. Run `python -m str2str_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the sampling path."
        )
    lib = ctypes.CDLL(p)
    for name, args in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.argtypes = args
        fn.restype = ctypes.c_longlong if name in _LL_RETURN else ctypes.c_int
    v = lib.s2s_abi_version()
    if v != ABI_VERSION:
        raise HipLibraryError(f"libstr2str_hip.so ABI {v} != expected {ABI_VERSION}; rebuild")
    if path is None:
        _lib = lib
    return lib


# ------------------------------------------------------------------------------------------ range guard of the f16x3 kernels
_range_flags = {}   # device index -> its eight int32 words, kept for the life of the process (captured HIP graphs hold the address)
RANGE_BITS = {1: "node GEMM", 2: "pack_planes", 4: "edge transition", 8: "edge embedding", 16: "IPA points", 32: "encoder attention"}
# kernel families as the sampler demotes them (str2str_amd/arith.py): flag bits -> family
RANGE_FAMILIES = {"node": 1 | 2 | 32, "edge_transition": 4, "edge_embed": 8, "ipa": 16}


def range_flag(device=None) -> torch.Tensor:
    """The range guard's buffer on ``device`` (default: the current one; csrc/range_flag.h): word 0 = one bit per kernel family whose
    split values reached 2^15 (half of f16's largest finite number) or were not finite; words 1..7 = magnitude buckets per family
    (``range_headroom``).  Every wrapper of an f16x3 entry point passes the current device's buffer with the call."""
    if not torch.cuda.is_available():
        raise HipLibraryError("the range flag lives on the HIP device")
    idx = None if device is None else torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    buf = _range_flags.get(idx)
    if buf is None:
        buf = _range_flags[idx] = torch.zeros(8, dtype=torch.int32, device=torch.device("cuda", idx))
    return buf


def range_flag_reset(device=None):
    range_flag(device).zero_()


def range_flag_read(device=None) -> int:
    """Synchronising read of the flag word (0 = every f16x3 launch since the last reset stayed in range)."""
    return int(range_flag(device)[0].item())


def range_flag_names(bits: int) -> str:
    return ", ".join(n for b, n in RANGE_BITS.items() if bits & b) or "none"


def range_families(bits: int):
    """Kernel families (keys of RANGE_FAMILIES) named by a flag word."""
    return [f for f, m in RANGE_FAMILIES.items() if bits & m]


def range_headroom(device=None) -> dict:
    """{family: upper bound of max |x| / 2^15} over every f16x3 launch since the last reset (synchronising read).  The kernels record
    maxima in power-of-two buckets from 2^8 up (nothing below: ordinary activations cost no atomic), so the figure is the bucket's
    upper edge: 2^-6 = "never reached 256", 1.0 = "in [2^14, 2^15)", 2.0 and 4.0 = the guard fired (4.0: 2^16 or more / not finite)."""
    words = range_flag(device).tolist()
    out = {}
    for fam, mask in RANGE_FAMILIES.items():
        top = -1
        for k in range(7):
            if mask >> k & 1 and words[1 + k]:
                top = max(top, int(words[1 + k]).bit_length() - 1)
        out[fam] = 2.0 ** (top + 9 - 15) if top >= 0 else 2.0 ** (8 - 15)
    return out


def _check(rc: int, what: str):
    if rc != 0:
        raise HipLibraryError(f"{what} failed with hipError_t {rc}")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t: torch.Tensor, dtype=torch.float32, name="tensor") -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipLibraryError(f"{name}: expected a tensor on the HIP device (no CPU fallback), got "
                              f"{getattr(t, 'device', type(t))}")
    if t.dtype != dtype:
        raise HipLibraryError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise HipLibraryError(f"{name}: expected a contiguous tensor")
    return t


def pack_weight(w: torch.Tensor, tile_major: bool = False) -> torch.Tensor:
    """[Mout, K] row-major -> kernel lane order (see include/str2str_hip.h).  Mout is zero-padded to
    a multiple of 32; K must be a multiple of 8.  ``tile_major`` orders fragments [t][s4] (a whole output
    tile is contiguous; s2s_edge_transition) instead of [s4][t]."""
    mout, k = w.shape
    if k % 8:
        raise ValueError("K must be a multiple of 8")
    pad = (-mout) % 32
    if pad:
        w = torch.cat([w, w.new_zeros(pad, k)], dim=0)
    t, s4 = w.shape[0] // 32, k // 8
    perm = (0, 2, 3, 1, 4) if tile_major else (2, 0, 3, 1, 4)
    return w.reshape(t, 32, s4, 2, 4).permute(*perm).contiguous().reshape(-1)


def fragment_order(w: torch.Tensor, kind: str) -> torch.Tensor:
    """[Mout, K] fp32 -> fp32 values in MFMA A-fragment order [K/16 k-steps][Mout/32 tiles][64 lanes][8] (v_mfma_f32_32x32x16_*).
    Element j of lane (m, g) in k-step ks is W[32t+m][k(ks,g,j)] with
      kind "row"  : k = 16*ks + 8*g + j                                   (B operand read from a memory row)
      kind "chain": k = 32*t' + (r&3) + 8*(r>>2) + 4*g, t' = ks>>1, r = 8*(ks&1) + j   (B operand = accumulator
                    registers of the previous layer in MFMA C layout)."""
    mout, k = w.shape
    if mout % 32 or k % 32:
        raise ValueError("Mout and K must be multiples of 32")
    T, KS = mout // 32, k // 16
    ks = torch.arange(KS)[:, None, None]
    g = torch.arange(2)[None, :, None]
    j = torch.arange(8)[None, None, :]
    if kind == "row":
        lab = 16 * ks + 8 * g + j
    elif kind == "chain":
        r = 8 * (ks & 1) + j
        lab = 32 * (ks >> 1) + (r & 3) + 8 * (r >> 2) + 4 * g
    else:
        raise ValueError(kind)
    wg = w.float()[:, lab.to(w.device)]  # [Mout, KS, 2, 8]
    return wg.reshape(T, 32, KS, 2, 8).permute(2, 0, 3, 1, 4).reshape(KS, T, 64, 8).contiguous()  # lane = 32*g + m


def pack_f16x2_layer(w: torch.Tensor, kind: str = "chain") -> torch.Tensor:
    """[Mout, K] fp32 -> f16 fragments [K/16][Mout/32][2 planes (W_h, W_l)][64][8] for v_mfma_f32_32x32x16_f16 A operands
    (lane / element order of ``fragment_order``): the f16 pair split of 2^5 w,  W_h = rn16(32 w),  W_l = rn16(32 w - W_h)  --
    the power of two keeps W_l in f16's normal range; the kernels take 2^-5 back in their epilogues (csrc/pair_mlp_f16.hip).
    A weight with |32 w| beyond f16's range cannot be packed: ``WeightRangeError`` (the modules then run on the fp32 kernels)."""
    wmax = float(w.detach().abs().max()) if w.numel() else 0.0
    if not (32.0 * wmax < 65504.0):
        raise WeightRangeError(f"|w| up to {wmax:.4g}: 32 w does not fit f16 (f16x3 weight packing)")
    planes = fragment_order(w, kind) * 32.0  # [KS, T, 64, 8] fp32 in fragment order
    h = planes.to(torch.float16)
    ls = (planes - h.float()).to(torch.float16)
    return torch.stack([h, ls], dim=2).contiguous()


def pack_f16x3_stream(w1_edge: torch.Tensor, w2: torch.Tensor, wf: torch.Tensor) -> torch.Tensor:
    """The weight stream of s2s_edge_transition_f16x3 as int16: 240 slots of 4 fragments ((W_h, W_l) of two (k-step, tile) units;
    8 slots = one 32 KiB stage, 30 stages) in the kernel's consumption order (csrc/pair_mlp_f16.hip):
      A_t (4 slots): layer-1 output tile t, k-step pairs (2s, 2s+1), fragments [k-step][plane];
      B_t (12 slots): layer-2 k-steps 2t + u (u = 0, 1) x output tile pairs 0..5, fragments [tile][plane]; B_11 pair-major
                      (pair b, then u): its first output tiles are complete early and their epilogue runs under the rest;
      F  (48 slots): final layer k-steps 0..23 x tile pairs 0..1;
    order  A_0 A_1 | B_0 A_2 | B_1 A_3 | ... | B_9 A_11 | B_10 B_11 | F."""
    l1, l2, lf = pack_f16x2_layer(w1_edge), pack_f16x2_layer(w2), pack_f16x2_layer(wf)
    A = lambda t: l1[:, t]
    B = lambda t: l2[2 * t:2 * t + 2]
    pieces = [A(0), A(1)]
    for t in range(10):
        pieces += [B(t), A(t + 2)]
    b11 = B(11)
    pieces += [B(10), b11.reshape(2, 6, 2, *b11.shape[2:]).transpose(0, 1), lf]   # B_11 tile-pair major (slots: pair b, then k-step u)
    blob = torch.cat([x.contiguous().reshape(-1) for x in pieces]).view(torch.int16).contiguous()
    assert blob.numel() * 2 == 30 * 32 * 1024, blob.numel()
    return blob


# ------------------------------------------------------------------------------------------ ops
class PairTiled:
    """A [B,N,N,128] pair tensor in the TILED layout the f16x3 pair kernels exchange among themselves (include/str2str_hip.h,
    "Pair-tensor layouts"): blocks of 32 consecutive pairs, inside a block [16 groups][2 halves][32 pairs][4 floats] -- the order in
    which a wavefront holds a 32-pair tile, so its loads and stores are whole cache lines.  ``buf`` is the flat fp32 storage
    (B N N rounded up to whole blocks); ``pair_tiled`` / ``pair_untiled`` convert from / to the reference's row-major tensor."""
    __slots__ = ("buf", "B", "N")

    def __init__(self, B: int, N: int, device=None, buf: Optional[torch.Tensor] = None):
        self.B, self.N = int(B), int(N)
        n = -(-(self.B * self.N * self.N) // 32) * 32 * 128
        self.buf = torch.empty(n, device=device, dtype=torch.float32) if buf is None else buf
        if self.buf.numel() != n or self.buf.dtype != torch.float32 or not self.buf.is_contiguous():
            raise HipLibraryError("PairTiled: buffer must be a contiguous fp32 tensor of whole 32-pair blocks")

    shape = property(lambda self: (self.B, self.N, self.N, 128))
    device = property(lambda self: self.buf.device)
    is_cuda = property(lambda self: self.buf.is_cuda)

    def data_ptr(self):
        return self.buf.data_ptr()

    def contiguous(self):
        return self


def pair_tiled(z: torch.Tensor) -> PairTiled:
    """Row-major [B,N,N,128] -> tiled (plain torch; conversion is for callers and tests, the kernels produce the layout themselves)."""
    B, N = z.shape[0], z.shape[1]
    M = B * N * N
    t = PairTiled(B, N, z.device)
    zp = torch.zeros(t.buf.numel() // 128, 128, device=z.device, dtype=torch.float32)
    zp[:M] = z.reshape(M, 128)
    t.buf.copy_(zp.view(-1, 32, 16, 2, 4).permute(0, 2, 3, 1, 4).reshape(-1))
    return t


def pair_untiled(t: PairTiled) -> torch.Tensor:
    M = t.B * t.N * t.N
    return t.buf.view(-1, 16, 2, 32, 4).permute(0, 3, 1, 2, 4).reshape(-1, 128)[:M].reshape(t.B, t.N, t.N, 128).contiguous()


def edge_transition_f16x3(edge, node_ab, node_p, wstream, b2, gamma, beta, mask, ln_eps=1e-5, out=None, proj=None,
                          out_layout: str = "rowmajor", prescale_exp: int = 0, ab_kernel_form: bool = False):
    """EdgeTransition on split-f16 MFMA (fp32-equivalent accuracy; csrc/pair_mlp_f16.hip); same contract as ``edge_transition``.
    ``proj`` = (31-stage stream = this layer's 30 stages (``pack_f16x3_stream``) + the next IPA block's projection stage
    (``pack_f16x2_layer``), bias64) also returns that block's (attn_bias [B,8,N,N], pair_z [B,N,N,32]).
    ``edge`` may be a ``PairTiled``; ``out_layout``: "rowmajor" (the reference's tensor), "tiled" (-> ``PairTiled``) or "none" (the pair
    vectors are not written: only with ``proj``, for the last EdgeTransition of a trunk; returns None in their place).
    ``prescale_exp`` = e (0 .. 15): the kernel keeps its hidden activations as f16 planes of 2^-e x the value (a block exponent: exact,
    same speed) -- what the sampler sets when the range guard reports hidden activations of 2^15 and beyond.
    ``node_ab`` [B,N,896] = [W1[:,128:256] n' + b1 | W1[:,256:] n' | Wf[:,256:] n' + bf] as ``EdgeTransition.node_parts`` gives it (the
    pair's per-node linear parts: row half and column half of the first layer, the j-side residual taken through the final layer incl.
    its bias); ``ab_kernel_form``: the column half and the third group already carry the accumulators' 2^5 (the trunk's per-node layers
    produce them so: no extra launch), see the C header."""
    lib = load_library()
    B, N = edge.shape[0], edge.shape[1]
    in_tiled = isinstance(edge, PairTiled)
    if not 0 <= int(prescale_exp) <= 15:
        raise HipLibraryError(f"edge_transition_f16x3: prescale_exp {prescale_exp} outside 0 .. 15")
    # C ABI: node_ab = [2^-e (A_i + b1) | 2^5 B_j | 2^(5-e) G_j] -- the row half at the planes' scale, the column half and the final layer's
    # start values at the accumulators' (the caller's job)
    if tuple(edge.shape) != (B, N, N, 128) or tuple(node_ab.shape) != (B, N, 896) or tuple(node_p.shape) != (B, N, 128):
        raise HipLibraryError(f"edge_transition_f16x3: bad shapes (edge {tuple(edge.shape)}, node_ab {tuple(node_ab.shape)}, node_p {tuple(node_p.shape)}): "
                              "edge is [B, N, N, 128], node_p [B, N, 128] and node_ab [B, N, 896] = EdgeTransition.node_parts (row half | column half | "
                              "j-side residual through the final layer; the 768-column form of earlier ABI versions is not accepted)")
    if not ab_kernel_form or prescale_exp:
        sc = node_ab.new_ones(896)
        sc[:384] = 2.0 ** -int(prescale_exp)
        sc[384:768] = 1.0 if ab_kernel_form else 32.0
        sc[768:] = (1.0 if ab_kernel_form else 32.0) * 2.0 ** -int(prescale_exp)
        node_ab = node_ab * sc
    if out_layout not in ("rowmajor", "tiled", "none") or (out_layout == "none" and proj is None):
        raise HipLibraryError(f"edge_transition_f16x3: out_layout {out_layout!r}" + (" needs proj" if out_layout == "none" else ""))
    _req(edge.buf if in_tiled else edge, name="edge")
    for n, t in (("node_ab", node_ab), ("node_p", node_p), ("b2", b2), ("gamma", gamma), ("beta", beta)):
        _req(t, name=n)
    pb = pbias = ppz = None
    if proj is not None:
        wstream, pb = proj
        _req(pb, name="proj.b64")
        pbias = torch.empty(B, 8, N, N, device=edge.device, dtype=torch.float32)
        ppz = torch.empty(B, N, N, 32, device=edge.device, dtype=torch.float32)
    _req(wstream, torch.int16, "wstream")
    if wstream.numel() * 2 != (31 if proj is not None else 30) * 32 * 1024:
        raise HipLibraryError("edge_transition_f16x3: weight stream has the wrong number of stages")
    if mask is not None:
        _req(mask, name="mask")
    if out_layout == "none":
        out = None
    elif out is None:
        out = PairTiled(B, N, edge.device) if out_layout == "tiled" else torch.empty(B, N, N, 128, device=edge.device, dtype=torch.float32)
    elif out.data_ptr() == edge.data_ptr():
        raise HipLibraryError("edge_transition: out may not alias edge")
    elif isinstance(out, PairTiled) != (out_layout == "tiled"):
        raise HipLibraryError("edge_transition_f16x3: out does not have the requested layout")
    io = (1 if in_tiled else 0) | {"rowmajor": 0, "tiled": 2, "none": 4}[out_layout]
    _check(_timed("s2s_edge_transition", lambda: lib.s2s_edge_transition_f16x3(
        _p(edge.buf if in_tiled else edge), _p(node_ab), _p(node_p), _p(wstream), _p(b2), _p(gamma), _p(beta),
        _p(mask),
        _p(out.buf if isinstance(out, PairTiled) else out), B, N, ln_eps, io, _p(pb), _p(pbias), _p(ppz), int(prescale_exp),
        _p(range_flag()), _stream())),
        "s2s_edge_transition_f16x3")
    return out if proj is None else (out, pbias, ppz)


def _proj_args(proj, B, N, dev):
    """(wp, b64) of the next IPA block -> (wp, b64, attn_bias_out, pair_z_out) or four Nones."""
    if proj is None:
        return None, None, None, None
    wp, b64 = proj
    _req(wp, name="proj.wp"); _req(b64, name="proj.b64")
    return (wp, b64, torch.empty(B, 8, N, N, device=dev, dtype=torch.float32),  # attention bias is head-major
            torch.empty(B, N, N, 32, device=dev, dtype=torch.float32))


def edge_transition(edge, node_ab, node_p, w1p, w2p, wfp, b2, bf, gamma, beta, mask, ln_eps=1e-5, out=None, proj=None):
    """-> out, or (out, attn_bias, pair_z) when ``proj`` = (packed Wcat, bias64) of the next IPA block is given."""
    lib = load_library()
    B, N = edge.shape[0], edge.shape[1]
    _req(edge, name="edge")
    if edge.shape != (B, N, N, 128) or node_ab.shape != (B, N, 768) or node_p.shape != (B, N, 128):
        raise HipLibraryError(f"edge_transition: bad shapes {tuple(edge.shape)} {tuple(node_ab.shape)} {tuple(node_p.shape)}")
    for n, t in (("node_ab", node_ab), ("node_p", node_p), ("w1p", w1p), ("w2p", w2p), ("wfp", wfp), ("b2", b2),
                 ("bf", bf), ("gamma", gamma), ("beta", beta)):
        _req(t, name=n)
    if mask is not None:
        _req(mask, name="mask")
    if out is None:
        out = torch.empty_like(edge)
    elif out.data_ptr() == edge.data_ptr():
        raise HipLibraryError("edge_transition: out may not alias edge")
    _req(out, name="out")
    pw, pb, pbias, ppz = _proj_args(proj, B, N, edge.device)
    _check(_timed("s2s_edge_transition", lambda: lib.s2s_edge_transition(
        _p(edge), _p(node_ab), _p(node_p), _p(w1p), _p(w2p), _p(wfp), _p(b2), _p(bf), _p(gamma), _p(beta), _p(mask),
        _p(out), B, N, ln_eps, _p(pw), _p(pb), _p(pbias), _p(ppz), _stream())), "s2s_edge_transition")
    return out if proj is None else (out, pbias, ppz)


def edge_embed(node_a, node_b, rel_table, bin_table, bin_lower, residue_idx, ca, w2p, w3p, b2, b3, gamma, beta, mask,
               rel_offset: int, ln_eps=1e-5, out=None, proj=None):
    lib = load_library()
    B, N = node_a.shape[0], node_a.shape[1]
    for n, t in (("node_a", node_a), ("node_b", node_b), ("rel_table", rel_table), ("bin_table", bin_table),
                 ("bin_lower", bin_lower), ("ca", ca), ("w2p", w2p), ("w3p", w3p), ("b2", b2), ("b3", b3),
                 ("gamma", gamma), ("beta", beta)):
        _req(t, name=n)
    _req(residue_idx, torch.int64, "residue_idx")
    if mask is not None:
        _req(mask, name="mask")
    if out is None:
        out = torch.empty(B, N, N, 128, device=node_a.device, dtype=torch.float32)
    pw, pb, pbias, ppz = _proj_args(proj, B, N, node_a.device)
    _check(lib.s2s_edge_embed(_p(node_a), _p(node_b), _p(rel_table), _p(bin_table), _p(bin_lower), _p(residue_idx), _p(ca),
                              _p(w2p), _p(w3p), _p(b2), _p(b3), _p(gamma), _p(beta), _p(mask), _p(out), B, N,
                              int(rel_offset), rel_table.shape[0], bin_table.shape[0], ln_eps, _p(pw), _p(pb), _p(pbias),
                              _p(ppz), _stream()), "s2s_edge_embed")
    return out if proj is None else (out, pbias, ppz)


def column_blocked(t: torch.Tensor) -> torch.Tensor:
    """[..., rows, 128] -> [..., 32, rows, 4]: element [c][row][q] = channel 4c + q (the gather layout of s2s_edge_embed_f16x3)."""
    *lead, rows, ch = t.shape
    return t.reshape(*lead, rows, ch // 4, 4).transpose(-3, -2).contiguous()


def pack_f16x3_embed_stream(w2: torch.Tensor, w3: torch.Tensor) -> torch.Tensor:
    """The 4-stage (32 KiB each) weight stream of s2s_edge_embed_f16x3: layer 2 then layer 3, [8 k-steps][4 tiles][(W_h, W_l)];
    the projection stage (``InvariantPointAttention._derived()['wp_f16x2']``) may be appended as the 5th."""
    blob = torch.cat([pack_f16x2_layer(w2, "chain").reshape(-1), pack_f16x2_layer(w3, "chain").reshape(-1)])
    blob = blob.view(torch.int16).contiguous()
    assert blob.numel() * 2 == 4 * 32 * 1024
    return blob


def edge_embed_f16x3(node_a, node_b, rel_table, bin_table, bin_lower, residue_idx, ca, wstream, b2, b3, gamma, beta, mask,
                     rel_offset: int, ln_eps=1e-5, out=None, proj=None, column_blocked_tables=False, out_layout: str = "rowmajor"):
    """Edge embedding on split-f16 MFMA (csrc/pair_mlp_f16.hip); ``proj`` = (5-stage stream, bias64) also returns (attn_bias, pair_z).
    node_b / rel_table / bin_table: [.., rows, 128], or already ``column_blocked`` ([.., 32, rows, 4]) with the flag set.
    ``out_layout`` "tiled" -> a ``PairTiled`` for ``edge_transition_f16x3``."""
    lib = load_library()
    B, N = node_a.shape[0], node_a.shape[1]
    if not column_blocked_tables:
        node_b, rel_table, bin_table = column_blocked(node_b), column_blocked(rel_table), column_blocked(bin_table)
    if node_b.shape != (B, 32, N, 4) or rel_table.shape[0] != 32 or bin_table.shape[0] != 32:
        raise HipLibraryError("edge_embed_f16x3: tables are not column-blocked [.., 32, rows, 4]")
    for n, t in (("node_a", node_a), ("node_b", node_b), ("rel_table", rel_table), ("bin_table", bin_table),
                 ("bin_lower", bin_lower), ("ca", ca), ("b2", b2), ("b3", b3), ("gamma", gamma), ("beta", beta)):
        _req(t, name=n)
    _req(residue_idx, torch.int64, "residue_idx")
    pb = pbias = ppz = None
    if proj is not None:
        wstream, pb = proj
        _req(pb, name="proj.b64")
        pbias = torch.empty(B, 8, N, N, device=node_a.device, dtype=torch.float32)
        ppz = torch.empty(B, N, N, 32, device=node_a.device, dtype=torch.float32)
    _req(wstream, torch.int16, "wstream")
    if wstream.numel() * 2 != (5 if proj is not None else 4) * 32 * 1024:
        raise HipLibraryError("s2s_edge_embed_f16x3: weight stream has the wrong number of stages")
    if mask is not None:
        _req(mask, name="mask")
    if out_layout not in ("rowmajor", "tiled"):
        raise HipLibraryError(f"edge_embed_f16x3: out_layout {out_layout!r}")
    tiled = out_layout == "tiled"
    if out is None:
        out = PairTiled(B, N, node_a.device) if tiled else torch.empty(B, N, N, 128, device=node_a.device, dtype=torch.float32)
    elif isinstance(out, PairTiled) != tiled:
        raise HipLibraryError("edge_embed_f16x3: out does not have the requested layout")
    _check(_timed("s2s_edge_embed", lambda: lib.s2s_edge_embed_f16x3(
        _p(node_a), _p(node_b), _p(rel_table), _p(bin_table), _p(bin_lower), _p(residue_idx), _p(ca), _p(wstream), _p(b2), _p(b3),
        _p(gamma), _p(beta), _p(mask), _p(out.buf if tiled else out), B, N, int(rel_offset), rel_table.shape[1], bin_table.shape[1],
        ln_eps, 1 if tiled else 0, _p(pb), _p(pbias), _p(ppz), _p(range_flag()), _stream())), "s2s_edge_embed_f16x3")
    return out if proj is None else (out, pbias, ppz)


def pair_project(edge, wp, bias64, attn_bias=None, pair_z=None):
    lib = load_library()
    B, N = edge.shape[0], edge.shape[1]
    _req(edge, name="edge"); _req(wp, name="wp"); _req(bias64, name="bias64")
    if attn_bias is None:
        attn_bias = torch.empty(B, 8, N, N, device=edge.device, dtype=torch.float32)  # head-major [B,H,N,N]
    if pair_z is None:
        pair_z = torch.empty(B, N, N, 32, device=edge.device, dtype=torch.float32)
    _check(lib.s2s_pair_project(_p(edge), _p(wp), _p(bias64), _p(attn_bias), _p(pair_z), B, N, _stream()), "s2s_pair_project")
    return attn_bias, pair_z


def ipa_prep_points(rigids7, q_pts_lin, kv_pts_lin, n_heads=8, n_qk=8, n_v=12):
    lib = load_library()
    B, N = rigids7.shape[0], rigids7.shape[1]
    for n, t in (("rigids7", rigids7), ("q_pts_lin", q_pts_lin), ("kv_pts_lin", kv_pts_lin)):
        _req(t, name=n)
    dev = rigids7.device
    q_pts = torch.empty(B, N, n_heads, n_qk * 3, device=dev, dtype=torch.float32)
    k_pts = torch.empty(B, N, n_heads, n_qk * 3, device=dev, dtype=torch.float32)
    v_pts = torch.empty(B, N, n_heads, 64, device=dev, dtype=torch.float32)
    _check(lib.s2s_ipa_prep_points(_p(rigids7), _p(q_pts_lin), _p(kv_pts_lin), _p(q_pts), _p(k_pts), _p(v_pts), B * N,
                                   n_heads, n_qk, n_v, 64, _stream()), "s2s_ipa_prep_points")
    return q_pts, k_pts, v_pts


def ipa_attention(q, kv, q_pts, k_pts, v_pts, attn_bias, pair_z, mask, rigids7, head_w_scaled, n_heads=8, c_hidden=256,
                  n_qk=8, n_v=12, c_pz=32, inf=1e5, eps=1e-8, out=None, logits_inplace=False):
    """Attention core + pair term.  ``attn_bias`` is head-major [B,H,N,N] (as ``pair_project`` writes it); with
    ``logits_inplace`` the masked logits overwrite it (the model does not reuse the bias).  Two launches:
    s2s_ipa_attention (o, o_pt, logits, row statistics) and s2s_ipa_opair (streams pair_z once for all heads)."""
    lib = load_library()
    B, N = mask.shape
    for n, t in (("q", q), ("kv", kv), ("q_pts", q_pts), ("k_pts", k_pts), ("v_pts", v_pts), ("attn_bias", attn_bias),
                 ("pair_z", pair_z), ("mask", mask), ("rigids7", rigids7), ("head_w", head_w_scaled)):
        _req(t, name=n)
    if attn_bias.shape != (B, n_heads, N, N) or pair_z.shape != (B, N, N, c_pz):
        raise HipLibraryError("ipa_attention: attn_bias must be [B,H,N,N] and pair_z [B,N,N,c_pz]")
    feat = n_heads * (c_hidden + 4 * n_v + c_pz)
    if out is None:
        out = torch.empty(B, N, feat, device=q.device, dtype=torch.float32)
    logits = attn_bias if logits_inplace else torch.empty_like(attn_bias)
    stats = torch.empty(B, n_heads, N, 2, device=q.device, dtype=torch.float32)

    def launch():
        rc = lib.s2s_ipa_attention(_p(q), _p(kv), _p(q_pts), _p(k_pts), _p(v_pts), _p(attn_bias), _p(logits), _p(stats),
                                   _p(mask), _p(rigids7), _p(head_w_scaled), _p(out), B, N, n_heads, c_hidden, n_qk, n_v,
                                   c_pz, inf, eps, _stream())
        if rc:
            return rc
        return lib.s2s_ipa_opair(_p(logits), _p(stats), _p(pair_z), _p(out), B, N, n_heads, c_pz, feat,
                                 n_heads * (c_hidden + 4 * n_v), N, _stream())

    _check(_timed("s2s_ipa_attention", launch), "s2s_ipa_attention/s2s_ipa_opair")
    return out


def padded_len(n_res: int) -> int:
    """n_res rounded up to the attention kernels' 32-residue tiles."""
    return (n_res + 31) // 32 * 32


def ipa_prep_points_f16(rigids7, q_pts_lin, kv_pts_lin, head_w_scaled, n_heads=8, n_qk=8, n_v=12, c_hidden=256, s_xp=None):
    """Global-frame points of a block as MFMA fragments (two f16 planes per fragment group) + the squared-norm terms of the logits
    (s2s_ipa_prep_points_f16).  ANY n_res: the arrays hold padded_len(n_res) rows per sample (padded rows: zero points, k2 = -1e9).
    rigids7 [B,N,7].  -> (qp_xp, kp_xp, vp_vf, q2, k2)
    With ``s_xp`` (packed planes of the block's input s [B*N, 256]; folded projections, ``fold_ipa_weights``) the same launch also
    writes the K / V operands every head shares: -> (..., k_shared, v_shared), k_shared = the rows of s_xp gathered into the padded
    per-sample layout (None when n_res % 32 == 0: s_xp itself is the K operand), v_shared = the same values as A fragments."""
    lib = load_library()
    _req(rigids7, name="rigids7"); _req(q_pts_lin, name="q_pts_lin"); _req(kv_pts_lin, name="kv_pts_lin")
    _req(head_w_scaled, name="head_w")
    if rigids7.ndim != 3:
        raise HipLibraryError("ipa_prep_points_f16: rigids7 must be [B,N,7]")
    B, N = rigids7.shape[:2]
    dev, rt = rigids7.device, B * padded_len(N) // 32
    qp = torch.empty(rt * n_heads * 2 * 2 * 64 * 8, dtype=torch.int16, device=dev)
    kp = torch.empty_like(qp)
    vp = torch.empty(rt * n_heads * 4 * 2 * 64 * 8, dtype=torch.int16, device=dev)
    q2 = torch.empty(rt, n_heads, 32, dtype=torch.float32, device=dev)
    k2 = torch.empty_like(q2)
    k_sh = v_sh = None
    if s_xp is not None:
        _req(s_xp, torch.int16, "s_xp")
        if s_xp.numel() != ((B * N + 31) // 32) * 32 * 256 * 2:
            raise HipLibraryError("ipa_prep_points_f16: s_xp must hold the packed planes of a [B*N, 256] activation")
        v_sh = torch.empty(rt * 32 * 256 * 2, dtype=torch.int16, device=dev)
        k_sh = None if N % 32 == 0 else torch.empty_like(v_sh)
    _check(lib.s2s_ipa_prep_points_f16(_p(rigids7), _p(q_pts_lin), _p(kv_pts_lin), _p(head_w_scaled), _p(qp), _p(kp), _p(vp), _p(q2),
                                       _p(k2), B, N, n_heads, n_qk, n_v, c_hidden, _p(s_xp), _p(k_sh), _p(v_sh), _p(range_flag()),
                                       _stream()),
           "s2s_ipa_prep_points_f16")
    return (qp, kp, vp, q2, k2) if s_xp is None else (qp, kp, vp, q2, k2, k_sh, v_sh)


def ipa_attention_f16(q_xp, k_xp, v_vf, points, attn_bias, pair_z, mask, rigids7, n_heads=8, c_hidden=256, n_qk=8, n_v=12,
                      c_pz=32, inf=1e5, eps=1e-8, logits_inplace=False):
    """Attention core on pre-split f16 pair operands + pair term (s2s_ipa_attention_f16w + s2s_ipa_opair), ANY n_res.
    ``points`` = ipa_prep_points_f16(...); for a ragged length the operand arrays hold padded_len(n_res) rows per sample (q/k from
    node_linear(row_map=...), v from node_linear_vfrag(row_map=...)) and the logits get their own padded buffer.
    -> (feats fp32 [B,N,feat] with the o_pt / o_pair columns valid, feats_xp packed planes with the o columns valid); the
    caller packs columns H*c_hidden.. of ``feats`` into ``feats_xp`` (ops.pack_planes) to complete linear_out's input."""
    lib = load_library()
    B, N = mask.shape
    qp, kp, vp, q2, k2 = points
    for n, t in (("attn_bias", attn_bias), ("pair_z", pair_z), ("mask", mask), ("rigids7", rigids7), ("q2", q2), ("k2", k2)):
        _req(t, name=n)
    for n, t in (("q_xp", q_xp), ("k_xp", k_xp), ("v_vf", v_vf), ("qp_xp", qp), ("kp_xp", kp), ("vp_vf", vp)):
        _req(t, torch.int16, n)
    NP = padded_len(N)
    if attn_bias.shape != (B, n_heads, N, N) or pair_z.shape != (B, N, N, c_pz):
        raise HipLibraryError("ipa_attention_f16: attn_bias must be [B,H,N,N] and pair_z [B,N,N,c_pz]")
    # K / V arrays of one head's size: one image serves every head (folded projections: both are the block's input s)
    n_kv = 1 if (k_xp.numel() * n_heads == q_xp.numel() and n_heads > 1) else n_heads
    if (q_xp.numel() != B * NP * n_heads * c_hidden * 2 or v_vf.numel() != k_xp.numel() or q2.numel() != B * NP * n_heads
            or k_xp.numel() * (n_heads // n_kv) != q_xp.numel()):
        raise HipLibraryError("ipa_attention_f16: operand arrays do not hold padded_len(n_res) rows per sample")
    feat = n_heads * (c_hidden + 4 * n_v + c_pz)
    out = torch.empty(B, N, feat, device=mask.device, dtype=torch.float32)
    out_xp = xp_alloc(B * N, feat, mask.device)
    if NP != N:
        logits = torch.empty(B, n_heads, NP, NP, device=mask.device, dtype=torch.float32)
    else:
        logits = attn_bias if logits_inplace else torch.empty_like(attn_bias)
    stats = torch.empty(B, n_heads, N, 2, device=mask.device, dtype=torch.float32)

    def launch():
        rc = lib.s2s_ipa_attention_f16w(_p(q_xp), _p(k_xp), _p(v_vf), _p(qp), _p(kp), _p(vp), _p(q2), _p(k2), _p(attn_bias), _p(logits),
                                        _p(stats), _p(mask), _p(rigids7), _p(out), _p(out_xp), feat // 16, B, N, n_heads, c_hidden,
                                        n_qk, n_v, c_pz, inf, eps, n_kv, _stream())
        if rc:
            return rc
        return lib.s2s_ipa_opair(_p(logits), _p(stats), _p(pair_z), _p(out), B, N, n_heads, c_pz, feat,
                                 n_heads * (c_hidden + 4 * n_v), NP, _stream())

    _check(_timed("s2s_ipa_attention", launch), "s2s_ipa_attention_f16w/s2s_ipa_opair")
    return out, out_xp


def rigid_compose_update(rigids7, update6, mask, out=None):
    """``update6``: [..., 6] contiguous, or a 2-D [n_frames, ld >= 6] fp32 buffer whose leading six columns are the update (the
    BackboneUpdate layer's padded output, read in place)."""
    lib = load_library()
    _req(rigids7, name="rigids7"); _req(update6, name="update6"); _req(mask, name="mask")
    n = rigids7.numel() // 7
    ld = update6.shape[-1] if (update6.ndim == 2 and update6.shape[0] == n) else 6
    if ld < 6 or update6.numel() != n * ld:
        raise HipLibraryError("rigid_compose_update: update6 must be [..., 6] or [n_frames, ld >= 6]")
    if out is None:
        out = torch.empty_like(rigids7)
    _check(lib.s2s_rigid_compose_update(_p(rigids7), _p(update6), _p(mask), _p(out), n, ld, _stream()),
           "s2s_rigid_compose_update")
    return out


def torsion_head(u, n_rows: int, normalize: bool = True, eps: float = 1e-8, gt_sin_cos=None, fixed_mask=None):
    """psi [n_rows, 2] from the torsion head's raw output ``u`` (2-D, leading two columns; normalised when ``normalize``) and, with
    ``gt_sin_cos`` (a [.., 2] view whose rows are ``gt_sin_cos.stride(-2)`` floats apart) + ``fixed_mask`` [n_rows], blended with the
    input torsion (s2s_torsion_head)."""
    lib = load_library()
    _req(u, name="u")
    if u.ndim != 2 or u.shape[0] != n_rows or u.shape[1] < 2:
        raise HipLibraryError("torsion_head: u must be [n_rows, ld >= 2]")
    gs = 0
    if gt_sin_cos is not None:
        if gt_sin_cos.dtype != torch.float32 or not gt_sin_cos.is_cuda or gt_sin_cos.shape[-1] != 2 or gt_sin_cos.stride(-1) != 1:
            raise HipLibraryError("torsion_head: gt_sin_cos must be a float32 device tensor [..., 2]")
        g2 = gt_sin_cos.reshape(-1, 2) if gt_sin_cos.is_contiguous() else gt_sin_cos
        gs = 2 if gt_sin_cos.is_contiguous() else gt_sin_cos.stride(-2)
        if not gt_sin_cos.is_contiguous() and any(gt_sin_cos.stride(d) != gt_sin_cos.stride(d + 1) * gt_sin_cos.shape[d + 1]
                                                  for d in range(gt_sin_cos.ndim - 2)):
            raise HipLibraryError("torsion_head: gt_sin_cos rows must be evenly strided")
        _req(fixed_mask, name="fixed_mask")
    out = torch.empty(n_rows, 2, device=u.device, dtype=torch.float32)
    _check(lib.s2s_torsion_head(_p(u), u.shape[1], int(bool(normalize)), _p(gt_sin_cos), gs, _p(fixed_mask), float(eps), _p(out), n_rows,
                                _stream()), "s2s_torsion_head")
    return out


def rigid_scale_trans(rigids7, scale: float, divide: bool = False, out=None):
    lib = load_library()
    _req(rigids7, name="rigids7")
    if out is None:
        out = torch.empty_like(rigids7)
    _check(lib.s2s_rigid_scale_trans(_p(rigids7), _p(out), rigids7.numel() // 7, scale, int(divide), _stream()),
           "s2s_rigid_scale_trans")
    return out


def _ensure_tables():
    dev = torch.cuda.current_device()
    if dev in _tables_loaded:
        return
    from .data import backbone_tables as bt

    lib = load_library()
    pos = np.ascontiguousarray(bt.BB_POS, dtype=np.float32)
    msk = np.ascontiguousarray(bt.BB_MASK, dtype=np.float32)
    grp = np.ascontiguousarray((bt.BB_GROUP == 3).astype(np.int32))
    frm = np.ascontiguousarray(bt.BB_FRAMES, dtype=np.float32)
    _check(lib.s2s_set_backbone_tables(pos.ctypes.data_as(_vp), msk.ctypes.data_as(_vp), grp.ctypes.data_as(_vp),
                                       frm.ctypes.data_as(_vp)), "s2s_set_backbone_tables")
    _tables_loaded.add(dev)


def frames_to_backbone(rigids7, psi, aatype=None, want_atom37=True, want_atom14=False):
    lib = load_library()
    _req(rigids7, name="rigids7"); _req(psi, name="psi")
    if aatype is not None:
        _req(aatype, torch.int64, "aatype")
    _ensure_tables()
    lead = rigids7.shape[:-1]
    dev = rigids7.device
    a37 = torch.empty(*lead, 37, 3, device=dev, dtype=torch.float32) if want_atom37 else None
    a14 = torch.empty(*lead, 5, 3, device=dev, dtype=torch.float32) if want_atom14 else None
    _check(lib.s2s_frames_to_backbone(_p(rigids7), _p(psi), _p(aatype), _p(a14), _p(a37), rigids7.numel() // 7, _stream()),
           "s2s_frames_to_backbone")
    return a37, a14


def se3_step(x0_7, xt_7, mask, diffuse_mask, params8, dt, coordinate_scaling: float = 0.1, probability_flow=True,
             center=True, noise_scale: float = 1.0, z_rot=None, z_trans=None, want_next=True, want_scores=False,
             rot_score_in=None, trans_score_in=None):
    """``dt``: the trajectory's step size (a float), or a float64 device tensor [B] with one step size per sample (a batch that holds
    trajectories of different t_delta)."""
    lib = load_library()
    B, N = mask.shape
    dt_vec = None
    if torch.is_tensor(dt):
        dt_vec = _req(dt, torch.float64, "dt")
        if dt_vec.shape != (B,):
            raise HipLibraryError("se3_step: a per-sample dt must be [B] float64")
        dt = 0.0
    for n, t in (("xt_7", xt_7), ("mask", mask), ("diffuse_mask", diffuse_mask), ("params8", params8)):
        _req(t, name=n)
    if rot_score_in is not None:
        _req(rot_score_in, torch.float64, "rot_score_in"); _req(trans_score_in, torch.float64, "trans_score_in")
    else:
        _req(x0_7, name="x0_7")
    if params8.shape != (B, 8):
        raise HipLibraryError("params8 must be [B, 8]")
    if not probability_flow:
        _req(z_rot, torch.float64, "z_rot"); _req(z_trans, torch.float64, "z_trans")
    dev = xt_7.device
    nxt = torch.empty(B, N, 7, device=dev, dtype=torch.float32) if want_next else None
    rs = torch.empty(B, N, 3, device=dev, dtype=torch.float64) if want_scores else None
    ts = torch.empty(B, N, 3, device=dev, dtype=torch.float64) if want_scores else None
    _check(lib.s2s_se3_step(_p(x0_7), _p(xt_7), _p(mask), _p(diffuse_mask), _p(params8), _p(z_rot), _p(z_trans), _p(rot_score_in),
                            _p(trans_score_in), _p(nxt),
                            _p(rs), _p(ts), B, N, float(dt), _p(dt_vec), float(coordinate_scaling), int(bool(probability_flow)),
                            int(center), float(noise_scale), _stream()), "s2s_se3_step")
    return nxt, rs, ts


def forward_marginal(rigids0_4x4, z_axis, u01, z_trans, cdf_rows, row_of_sample, omega_grid, params2, diffuse_mask=None,
                     coordinate_scaling: float = 0.1):
    """Forward marginal (``rigids0_4x4`` [B,N,4,4]) or prior sample (``None``) from caller-drawn noise -> rigids_t7 [B,N,7]."""
    lib = load_library()
    B, N = u01.shape
    for n, t in (("z_axis", z_axis), ("u01", u01), ("z_trans", z_trans), ("omega_grid", omega_grid)):
        _req(t, name=n)
    _req(cdf_rows, torch.float64, "cdf_rows"); _req(row_of_sample, torch.int32, "row_of_sample")
    if z_axis.shape != (B, N, 3) or z_trans.shape != (B, N, 3) or cdf_rows.ndim != 2 or cdf_rows.shape[1] != omega_grid.numel() \
            or row_of_sample.shape != (B,):
        raise HipLibraryError("forward_marginal: bad shapes")
    if rigids0_4x4 is not None:
        _req(rigids0_4x4, name="rigids0_4x4"); _req(params2, name="params2")
        if rigids0_4x4.shape != (B, N, 4, 4) or params2.shape != (B, 2):
            raise HipLibraryError("forward_marginal: rigids0_4x4 must be [B,N,4,4] and params2 [B,2]")
    if diffuse_mask is not None:
        _req(diffuse_mask, name="diffuse_mask")
    out = torch.empty(B, N, 7, device=u01.device, dtype=torch.float32)
    _check(lib.s2s_forward_marginal(_p(rigids0_4x4), _p(z_axis), _p(u01), _p(z_trans), _p(cdf_rows), _p(row_of_sample),
                                    _p(omega_grid), omega_grid.numel(), _p(params2), _p(diffuse_mask), float(coordinate_scaling),
                                    _p(out), B, N, _stream()), "s2s_forward_marginal")
    return out


# ------------------------------------------------------------------------------------------ per-node dense layers
NODE_TG = (10, 8, 6, 5, 4, 2, 1)   # tiles of 32 output columns per workgroup the kernel is instantiated for


def node_tiles(n_out: int, whole_row: bool = False) -> int:
    """Tiles per column block for an ``n_out``-wide layer (``whole_row``: one block must hold the row, e.g. for LayerNorm)."""
    if n_out % 32:
        raise ValueError("n_out must be a multiple of 32 (pad the weight)")
    t = n_out // 32
    if whole_row:
        if t not in NODE_TG:
            raise HipLibraryError(f"no node_linear instantiation holds a whole row of {n_out} columns")
        return t
    return next(g for g in NODE_TG if t % g == 0)


def pack_node_weight(w: torch.Tensor, tiles_per_block: int) -> torch.Tensor:
    """[n_out, k_in] fp32 -> int16 blob [n_out/(32 TG)][k_in/16][TG][2][64][8] of chain-ordered f16 A fragments (W_h, W_l)
    (s2s_node_linear).  n_out is zero-padded to a multiple of 32 first."""
    n_out, k = w.shape
    pad = (-n_out) % 32
    if pad:
        w = torch.cat([w, w.new_zeros(pad, k)], dim=0)
    if k % 32 or (w.shape[0] // 32) % tiles_per_block:
        raise ValueError("k_in must be a multiple of 32 and n_out/32 of tiles_per_block")
    fr = pack_f16x2_layer(w.float(), "chain")                       # [KS, T, 2, 64, 8]
    KS, T = fr.shape[:2]
    fr = fr.reshape(KS, T // tiles_per_block, tiles_per_block, 2, 64, 8).permute(1, 0, 2, 3, 4, 5)
    return fr.contiguous().view(torch.int16).reshape(-1)


def pack_node_weight_f32(w: torch.Tensor, tiles_per_block: int) -> torch.Tensor:
    """[n_out, k_in] fp32 -> fp32 blob [n_out/(32 TG)][k_in/8][TG][64][4] in the ``pack_weight`` lane order (s2s_node_linear_f32)."""
    n_out, k = w.shape
    pad = (-n_out) % 32
    if pad:
        w = torch.cat([w, w.new_zeros(pad, k)], dim=0)
    if k % 8 or (w.shape[0] // 32) % tiles_per_block:
        raise ValueError("k_in must be a multiple of 8 and n_out/32 of tiles_per_block")
    T, S4 = w.shape[0] // 32, k // 8
    fr = w.float().reshape(T // tiles_per_block, tiles_per_block, 32, S4, 2, 4).permute(0, 3, 1, 4, 2, 5)   # [cb, s4, t, g, m, q]
    return fr.contiguous().reshape(-1)


def pack_node_layer(w: torch.Tensor, bias, whole_row: bool = False) -> dict:
    """Everything ``node_apply`` needs of one nn.Linear of the node stream: tile grouping, padded bias, and the packed weights of
    BOTH arithmetics, built on first use ("w": f16x3 fragments, "w32": exact fp32)."""
    n_out, k = w.shape
    n_pad = -(-n_out // 32) * 32
    tg = node_tiles(n_pad, whole_row=whole_row)
    b = w.new_zeros(n_pad, dtype=torch.float32)
    if bias is not None:
        b[:n_out] = bias.detach().float()
    # "tg_s": the column block for SMALL row counts (a few thousand rows: the reference's default inference block).  There a launch is one
    # workgroup's latency chain, and narrower blocks mean more workgroups with shorter k-steps and epilogues (profiles/
    # r04_node_gemm_small_m.txt: 320 -> 960 columns 29.5 -> 19.8 us, 256 -> 512 20.4 -> 13.0 us at 5120 rows); with rows to spare the wide
    # block wins (every weight stage serves more MFMAs).  A layer that needs the whole row in one block (LayerNorm) has no choice.
    t = n_pad // 32
    tg_s = tg if whole_row else (2 if t % 2 == 0 else tg)
    return _NodeLayer({"b": b.contiguous(), "n": n_pad, "k": k, "tg": tg, "tg_s": tg_s}, w.detach())


class _NodeLayer(dict):
    def __init__(self, d, w):
        super().__init__(d)
        self._w = w

    def __missing__(self, key):
        if key == "w":
            self[key] = pack_node_weight(self._w.float(), self["tg"])
        elif key == "w_s":
            self[key] = self["w"] if self["tg_s"] == self["tg"] else pack_node_weight(self._w.float(), self["tg_s"])
        elif key == "w_row":   # one column block = the whole row (s2s_node_chain)
            self[key] = self["w"] if self["tg"] == self["n"] // 32 else pack_node_weight(self._w.float(), self["n"] // 32)
        elif key == "w32":
            self[key] = pack_node_weight_f32(self._w.float(), self["tg"])
        else:
            raise KeyError(key)
        return self[key]


def xp_alloc(n_rows: int, k: int, device) -> torch.Tensor:
    """Packed-plane activation buffer for [n_rows, k] (int16 storage; two f16 planes per k-step; see include/str2str_hip.h)."""
    return torch.empty(((n_rows + 31) // 32) * (k // 16) * 2 * 64 * 8, dtype=torch.int16, device=device)


def act_alloc(n_rows: int, k: int, device, arith: str) -> torch.Tensor:
    """Activation buffer of the node stream: packed f16 planes ("f16x3") or fp32 row-major [n_rows, k] ("f32")."""
    return xp_alloc(n_rows, k, device) if arith == "f16x3" else torch.empty(n_rows, k, device=device, dtype=torch.float32)


def pack_planes(x2d: torch.Tensor, col0: int = 0, n_cols: Optional[int] = None, out=None, out_k: Optional[int] = None,
                k0: int = 0, row_scale=None):
    """fp32 [M, ld] (columns col0 .. col0 + n_cols) -> XP planes, optionally into columns k0.. of a wider XP buffer."""
    lib = load_library()
    _req(x2d, name="x")
    M, ld = x2d.shape
    n_cols = ld - col0 if n_cols is None else n_cols
    out_k = n_cols if out_k is None else out_k
    if out is None:
        out = xp_alloc(M, out_k, x2d.device)
    if row_scale is not None:
        _req(row_scale, name="row_scale")
    _check(lib.s2s_pack_planes(_p(x2d), M, ld, col0, n_cols, _p(out), out_k // 16, k0 // 16, _p(row_scale), _p(range_flag()),
                               _stream()), "s2s_pack_planes")
    return out


def to_act(x2d: torch.Tensor, arith: str) -> torch.Tensor:
    """fp32 [M, K] -> the node stream's activation format: packed planes ("f16x3") or the tensor itself ("f32")."""
    return pack_planes(x2d) if arith == "f16x3" else _req(x2d, name="x")


def node_linear(xp, wpk, bias, n_rows: int, k_in: int, n_out: int, tiles: int, *, pre_scale=None, relu=False, pre_mask=None,
                residual=None, ln=None, post_mask=None, out_f32=None, out_col0: int = 0, want_f32=True, out_xp=None,
                out_xp_k: Optional[int] = None, out_xp_k0: int = 0, want_xp=False, row_map: Optional[tuple] = None):
    """One fused per-node layer on split-f16 MFMA (s2s_node_linear).  ``residual`` [n_rows, ld] fp32 (its leading n_out columns are
    added); ``ln`` = (gamma, beta, eps); ``out_f32`` a preallocated [n_rows, ld] buffer written at ``out_col0`` (allocated
    [n_rows, n_out] when ``want_f32``); ``out_xp`` likewise for the packed planes.  ``row_map`` = (n_pad, n_src): ``n_rows`` counts
    OUTPUT rows = samples * n_pad, output row (sample, n) is computed from input row sample * n_src + min(n, n_src - 1) (per-sample
    padding to whole 32-row tiles for the attention kernel).  -> (out_f32 or None, out_xp or None)."""
    lib = load_library()
    _req(xp, torch.int16, "xp"); _req(wpk, torch.int16, "w_packed")
    dev = xp.device
    map_pad, map_src = row_map if row_map is not None else (0, 0)
    in_rows = n_rows // map_pad * map_src if map_pad else n_rows
    for n, t in (("bias", bias), ("pre_scale", pre_scale), ("pre_mask", pre_mask), ("residual", residual), ("post_mask", post_mask)):
        if t is not None:
            _req(t, name=n)
    if xp.numel() != ((in_rows + 31) // 32) * (k_in // 16) * 1024 or wpk.numel() != n_out * k_in * 2:
        raise HipLibraryError(f"node_linear: operand sizes do not match M={in_rows} K={k_in} N={n_out}")
    if out_f32 is None and want_f32:
        out_f32 = torch.empty(n_rows, n_out, device=dev, dtype=torch.float32)
    if out_f32 is not None:
        _req(out_f32, name="out_f32")
    if out_xp is None and want_xp:
        out_xp_k = n_out if out_xp_k is None else out_xp_k
        out_xp = xp_alloc(n_rows, out_xp_k, dev)
    if out_xp is not None:
        out_xp_k = n_out if out_xp_k is None else out_xp_k
        _req(out_xp, torch.int16, "out_xp")
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    if ln is not None:
        _req(g, name="ln.gamma"); _req(b, name="ln.beta")
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_linear(
        _p(xp), _p(wpk), _p(bias), n_rows, k_in, n_out, tiles, _p(pre_scale), int(bool(relu)), _p(pre_mask), _p(residual),
        residual.shape[-1] if residual is not None else 0, _p(g), _p(b), float(eps), _p(post_mask), _p(out_f32),
        out_f32.shape[-1] if out_f32 is not None else 0, out_col0, _p(out_xp), (out_xp_k or 0) // 16, out_xp_k0 // 16,
        map_pad, map_src, _p(range_flag()), _stream()), flops=2 * n_rows * k_in * n_out), "s2s_node_linear")
    return out_f32, out_xp


def node_linear_f32(x, wpk32, bias, n_rows: int, k_in: int, n_out: int, tiles: int, *, pre_scale=None, relu=False, pre_mask=None,
                    residual=None, ln=None, post_mask=None, out=None, out_col0: int = 0):
    """The same layer on exact fp32 MFMA (s2s_node_linear_f32): x fp32 [n_rows, ld >= k_in], ``wpk32`` = pack_node_weight_f32;
    -> out fp32 (allocated [n_rows, n_out] unless given: written at ``out_col0``)."""
    lib = load_library()
    _req(x, name="x"); _req(wpk32, name="w_packed_f32")
    if x.ndim != 2 or x.shape[0] != n_rows or x.shape[1] < k_in or wpk32.numel() != n_out * k_in:
        raise HipLibraryError(f"node_linear_f32: operand sizes do not match M={n_rows} K={k_in} N={n_out}")
    for n, t in (("bias", bias), ("pre_scale", pre_scale), ("pre_mask", pre_mask), ("residual", residual), ("post_mask", post_mask)):
        if t is not None:
            _req(t, name=n)
    if out is None:
        out = torch.empty(n_rows, n_out, device=x.device, dtype=torch.float32)
    _req(out, name="out")
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    if ln is not None:
        _req(g, name="ln.gamma"); _req(b, name="ln.beta")
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_linear_f32(
        _p(x), x.shape[1], _p(wpk32), _p(bias), n_rows, k_in, n_out, tiles, _p(pre_scale), int(bool(relu)), _p(pre_mask), _p(residual),
        residual.shape[-1] if residual is not None else 0, _p(g), _p(b), float(eps), _p(post_mask), _p(out), out.shape[-1], out_col0,
        _stream()), flops=2 * n_rows * k_in * n_out), "s2s_node_linear_f32")
    return out


SMALL_ROWS = 8192        # at or below: a long contraction with a row-normalising epilogue runs as narrow GEMM + LayerNorm (node_apply)
NARROW_MAX_WORK = 24 << 20   # rows x output columns up to which the narrow column blocks ("tg_s") of a layer are the faster form
#   (tools/node_gemm_bench.py --tg 2 against the default, profiles/r04_node_gemm_small_m.txt: 2048 columns win up to ~10 k rows and
#    lose from ~24 k, 512 .. 960 columns still win at 24 k rows)


def small_rows_variant(layer: dict, n_rows: int):
    """-> (key of the packed weights, tiles per column block) a layer runs with at this row count."""
    if n_rows * layer["n"] <= NARROW_MAX_WORK and layer.get("tg_s", layer["tg"]) != layer["tg"]:
        return "w_s", layer["tg_s"]
    return "w", layer["tg"]


def embed_assemble(t_img, node_const, fa, fb, n_samples: int, n_res: int, planes: bool, b_col_blocked: bool):
    """The embedder's per-evaluation assembly (s2s_embed_assemble): -> (h as packed planes [M,256] or fp32, node_a [B,L,128], node_b in
    ``fb``'s layout) from the chunk's timestep image ``t_img`` [512] -- or one image per sample, [n_samples, 512] -- and the cached
    per-target terms."""
    lib = load_library()
    for n, t in (("t_img", t_img), ("node_const", node_const), ("fa", fa), ("fb", fb)):
        _req(t, name=n)
    M, dev = n_samples * n_res, t_img.device
    if t_img.numel() not in (512, 512 * n_samples) or node_const.numel() not in (M * 256, n_res * 256) or fa.numel() != M * 128 or fb.numel() != M * 128:
        raise HipLibraryError("embed_assemble: bad shapes")
    h = xp_alloc(M, 256, dev) if planes else torch.empty(M, 256, device=dev, dtype=torch.float32)
    node_a, node_b = torch.empty(n_samples, n_res, 128, device=dev, dtype=torch.float32), torch.empty_like(fb)
    _check(lib.s2s_embed_assemble(_p(t_img), t_img.numel() // 512 if t_img.numel() != 512 else 1, _p(node_const), node_const.numel() // 256, _p(fa), _p(fb), M, n_res, _p(h) if planes else None,
                                  None if planes else _p(h), _p(node_a), _p(node_b), int(b_col_blocked), _p(range_flag()), _stream()), "s2s_embed_assemble")
    return h, node_a, node_b


def row_layernorm(x, n_rows: int, n_cols: int, gamma, beta, eps: float, post_mask=None, out_f32=None, out_col0: int = 0, want_f32=True,
                  out_xp=None, out_xp_k: Optional[int] = None, out_xp_k0: int = 0, want_xp=False):
    """LayerNorm (+ post mask) of the leading ``n_cols`` columns of fp32 rows with the node GEMM's epilogue code (s2s_row_layernorm):
    the second half of a layer whose GEMM ran without its LayerNorm.  Same output conventions as ``node_linear``."""
    lib = load_library()
    _req(x, name="x"); _req(gamma, name="ln.gamma"); _req(beta, name="ln.beta")
    dev = x.device
    if post_mask is not None:
        _req(post_mask, name="post_mask")
    if out_f32 is None and want_f32:
        out_f32 = torch.empty(n_rows, n_cols, device=dev, dtype=torch.float32)
    if out_xp is None and want_xp:
        out_xp_k = n_cols if out_xp_k is None else out_xp_k
        out_xp = xp_alloc(n_rows, out_xp_k, dev)
    if out_xp is not None:
        out_xp_k = n_cols if out_xp_k is None else out_xp_k
    _check(_timed("s2s_node_linear", lambda: lib.s2s_row_layernorm(
        _p(x), x.shape[-1], n_rows, n_cols, _p(gamma), _p(beta), float(eps), _p(post_mask), _p(out_f32),
        out_f32.shape[-1] if out_f32 is not None else 0, out_col0, _p(out_xp), (out_xp_k or 0) // 16, out_xp_k0 // 16, _p(range_flag()),
        _stream())),
        "s2s_row_layernorm")
    return out_f32, out_xp


def node_apply(x, layer: dict, n_rows: int, *, out_f32=None, out_col0: int = 0, want_f32=True, out_xp=None, out_xp_k=None,
               out_xp_k0: int = 0, want_xp=False, **epilogue):
    """One layer of the node stream in the arithmetic of its INPUT: ``x`` packed f16 planes (int16) -> s2s_node_linear, ``x`` fp32
    [n_rows, K] -> s2s_node_linear_f32.  ``layer`` = pack_node_layer(...).  Same calling convention and return value
    (fp32 output or None, activation-format output or None) in both; in the fp32 arithmetic the two outputs are the same tensor
    (``out_xp``, an fp32 buffer there, is written at column ``out_xp_k0`` when no ``out_f32`` is given)."""
    T = torch.ops.str2str_amd
    ep = dict(epilogue)
    ln = ep.pop("ln", None)
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    row_map = ep.pop("row_map", None)
    flat = (ep.pop("pre_scale", None), bool(ep.pop("relu", False)), ep.pop("pre_mask", None), ep.pop("residual", None), g, b, float(eps),
            ep.pop("post_mask", None))
    if ep:
        raise TypeError(f"node_apply: unexpected arguments {sorted(ep)}")
    if x.dtype == torch.int16 and g is not None and n_rows <= SMALL_ROWS and layer["k"] >= 1024 and layer["n"] in (256, 320) and row_map is None:
        # a long contraction on few rows whose epilogue normalises over the row (linear_out, K = 2688): one column block per row tile
        # is K / 16 serial k-steps of 24 MFMAs on 1 / 6 of the chip; GEMM in narrow blocks + the LayerNorm on its own is the same
        # arithmetic (s2s_row_layernorm) in a third of the time
        if "w_n" not in layer:
            layer["w_n"] = pack_node_weight(layer._w.float(), 2)
        pre = torch.empty(n_rows, layer["n"], device=x.device, dtype=torch.float32)
        T.node_linear(x, layer["w_n"], layer["b"], n_rows, layer["k"], layer["n"], 2, flat[0], flat[1], flat[2], flat[3], None, None, 0.0, None,
                      pre, 0, True, None, -1, 0, False, 0, 0)
        return T.row_layernorm(pre, n_rows, layer["n"], g, b, float(eps), flat[7], out_f32, out_col0, want_f32, out_xp,
                               -1 if out_xp_k is None else out_xp_k, out_xp_k0, want_xp)
    if x.dtype == torch.int16:
        mp, ms = row_map if row_map is not None else (0, 0)
        wk, tg = small_rows_variant(layer, n_rows)
        return T.node_linear(x, layer[wk], layer["b"], n_rows, layer["k"], layer["n"], tg, *flat, out_f32, out_col0, want_f32,
                             out_xp, -1 if out_xp_k is None else out_xp_k, out_xp_k0, want_xp, mp, ms)
    if row_map is not None:
        raise HipLibraryError("node_apply: the row map belongs to the f16 attention operands")
    if out_f32 is not None:
        out, col0 = out_f32, out_col0
        if out_xp is not None and out_xp is not out_f32:
            raise HipLibraryError("node_apply (fp32): one output buffer")
    else:
        out, col0 = out_xp, out_xp_k0
    y = T.node_linear_f32(x, layer["w32"], layer["b"], n_rows, layer["k"], layer["n"], layer["tg"], *flat, out, col0)
    return y, y


def node_linear_vfrag(xp, wpk, bias, n_rows: int, k_in: int, n_out: int, tiles_per_head: int = 8, out=None,
                      row_map: Optional[tuple] = None):
    """Projection stored as MFMA A fragments of f16 pairs over 32-row tiles (s2s_node_linear_vfrag; the value projection of the IPA).
    -> int16 buffer [row tiles][heads][tiles_per_head][2][2][64][8]."""
    lib = load_library()
    _req(xp, torch.int16, "xp"); _req(wpk, torch.int16, "w_packed")
    if bias is not None:
        _req(bias, name="bias")
    n_el = ((n_rows + 31) // 32) * (n_out // 32) * 2 * 2 * 64 * 8
    if out is None:
        out = torch.empty(n_el, dtype=torch.int16, device=xp.device)
    _req(out, torch.int16, "out_vf")
    map_pad, map_src = row_map if row_map is not None else (0, 0)
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_linear_vfrag(_p(xp), _p(wpk), _p(bias), n_rows, k_in, n_out, tiles_per_head,
                                                                       _p(out), map_pad, map_src, _p(range_flag()), _stream()),
                  flops=2 * n_rows * k_in * n_out),
           "s2s_node_linear_vfrag")
    return out


class _NodeProblem(ctypes.Structure):   # s2s_node_problem (include/str2str_hip.h)
    _fields_ = [("xp", ctypes.c_void_p), ("w_packed", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("n_rows", ctypes.c_longlong),
                ("k_in", ctypes.c_int), ("n_out", ctypes.c_int), ("tiles_per_block", ctypes.c_int), ("vfrag_tiles_per_head", ctypes.c_int),
                ("out_f32", ctypes.c_void_p), ("out_ld", ctypes.c_int), ("out_col0", ctypes.c_int), ("out_xp", ctypes.c_void_p),
                ("out_xp_ksteps", ctypes.c_int), ("out_xp_kstep0", ctypes.c_int), ("out_vf", ctypes.c_void_p), ("map_pad", ctypes.c_int),
                ("map_src", ctypes.c_int), ("relu", ctypes.c_int), ("pre_scale", ctypes.c_void_p)]


def node_linear_multi(xp, w, bias, pre_scale, dims, out_f32, out_xp):
    """Up to six node layers that read the same packed planes ``xp``, in ONE launch (s2s_node_linear_multi).  Lists, one entry per
    layer: ``w`` (packed weights), ``bias``, ``pre_scale`` ([n_rows] row scale or an empty tensor), ``out_f32`` / ``out_xp`` (the
    caller's output buffers, written in place; an empty tensor = that output is not wanted), and in ``dims`` nine ints per layer:
    n_rows, k_in, n_out, tiles_per_block, out_ld (row stride of out_f32), out_col0, out_xp_k (width of the planes buffer), out_xp_k0, relu.
    Bitwise what the separate s2s_node_linear launches give."""
    lib = load_library()
    _req(xp, torch.int16, "xp")
    n = len(w)
    if not (1 <= n <= 6) or any(len(x) != n for x in (bias, pre_scale, out_f32, out_xp)) or len(dims) != 9 * n:
        raise HipLibraryError("node_linear_multi: 1 .. 6 layers, one entry per layer in every list, nine ints per layer")
    arr = (_NodeProblem * n)()
    for i in range(n):
        rows, k, nn, tg, ld, c0, xk, xk0, relu = (int(v) for v in dims[9 * i:9 * i + 9])
        _req(w[i], torch.int16, "w"); _req(bias[i], name="bias")
        p = arr[i]
        p.xp, p.w_packed, p.bias = xp.data_ptr(), w[i].data_ptr(), bias[i].data_ptr()
        p.n_rows, p.k_in, p.n_out, p.tiles_per_block, p.relu = rows, k, nn, tg, relu
        if pre_scale[i].numel():
            _req(pre_scale[i], name="pre_scale")
            p.pre_scale = pre_scale[i].data_ptr()
        if out_f32[i].numel():
            _req(out_f32[i], name="out_f32")
            p.out_f32, p.out_ld, p.out_col0 = out_f32[i].data_ptr(), ld, c0
        if out_xp[i].numel():
            _req(out_xp[i], torch.int16, "out_xp")
            p.out_xp, p.out_xp_ksteps, p.out_xp_kstep0 = out_xp[i].data_ptr(), xk // 16, xk0 // 16
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_linear_multi(ctypes.byref(arr), n, _p(range_flag()), _stream()),
                  flops=sum(2 * arr[i].n_rows * arr[i].k_in * arr[i].n_out for i in range(n))), "s2s_node_linear_multi")


def ipa_projections(s_xp, q, k, v, qp, kvp, n_rows: int, n_rows_padded: int, row_map: Optional[tuple] = None, tiles_per_head: int = 8):
    """The projections of an IPA block (reference ipa.py:131-171) in ONE launch (s2s_node_linear_multi): ``q`` / ``k`` -> packed
    planes over ``n_rows_padded`` rows (the attention kernel's per-sample padded layout when ``row_map`` = (n_pad, n_src)), ``v`` -> A
    fragments over the same rows, ``qp`` / ``kvp`` (point projections) -> fp32 [n_rows, n].  Each argument is a ``pack_node_layer``
    dict; ``k`` / ``v`` may be None (folded projections, ``fold_ipa_weights``: the attention reads s itself).
    -> (q_xp, k_xp, v_vf, qp_f32, kvp_f32), None for an absent layer; bitwise what the separate launches give."""
    lib = load_library()
    _req(s_xp, torch.int16, "xp")
    dev = s_xp.device
    mp, ms = row_map if row_map is not None else (0, 0)
    q_xp = xp_alloc(n_rows_padded, q["n"], dev)
    k_xp = xp_alloc(n_rows_padded, k["n"], dev) if k is not None else None
    v_vf = (torch.empty(((n_rows_padded + 31) // 32) * (v["n"] // 32) * 2 * 2 * 64 * 8, dtype=torch.int16, device=dev)
            if v is not None else None)
    qp_o = torch.empty(n_rows, qp["n"], device=dev, dtype=torch.float32)
    kvp_o = torch.empty(n_rows, kvp["n"], device=dev, dtype=torch.float32)
    arr = (_NodeProblem * 5)()
    n = 0

    def fill(layer, rows, **kw):
        nonlocal n
        p = arr[n]
        n += 1
        p.xp, p.w_packed, p.bias = s_xp.data_ptr(), layer["w"].data_ptr(), layer["b"].data_ptr()   # (the caller picked the variant: "w" / "tg")
        p.n_rows, p.k_in, p.n_out, p.tiles_per_block = rows, layer["k"], layer["n"], layer["tg"]
        for name, val in kw.items():
            setattr(p, name, val)

    fill(q, n_rows_padded, out_xp=q_xp.data_ptr(), out_xp_ksteps=q["n"] // 16, map_pad=mp, map_src=ms)
    if k is not None:
        fill(k, n_rows_padded, out_xp=k_xp.data_ptr(), out_xp_ksteps=k["n"] // 16, map_pad=mp, map_src=ms)
    if v is not None:
        fill(v, n_rows_padded, vfrag_tiles_per_head=tiles_per_head, out_vf=v_vf.data_ptr(), map_pad=mp, map_src=ms)
    fill(qp, n_rows, out_f32=qp_o.data_ptr(), out_ld=qp["n"])
    fill(kvp, n_rows, out_f32=kvp_o.data_ptr(), out_ld=kvp["n"])
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_linear_multi(ctypes.byref(arr), n, _p(range_flag()), _stream()),
                  flops=sum(2 * arr[i].n_rows * arr[i].k_in * arr[i].n_out for i in range(n))), "s2s_node_linear_multi")
    return q_xp, k_xp, v_vf, qp_o, kvp_o


class _ChainLayer(ctypes.Structure):   # s2s_chain_layer (include/str2str_hip.h)
    _fields_ = [("w_packed", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("relu", ctypes.c_int)]


CHAIN_WIDTHS = (256, 320)


def node_chain(xp, w_row, bias, relu, n_rows: int, width: int, pre_mask=None, residual=None, ln_gamma=None, ln_beta=None, ln_eps: float = 0.0,
               post_mask=None, out_f32=None, out_col0: int = 0, want_f32=True, out_xp=None, out_xp_k: Optional[int] = None,
               out_xp_k0: int = 0, want_xp=False, k_in0: Optional[int] = None, mid_residual=None, mid_out_f32=None, mid_ln=None):
    """2 .. 4 layers of one output width (``width`` = 256 | 320) in one launch (s2s_node_chain): relu?(W x + b) between, the last layer with
    ``node_linear``'s epilogue and outputs; hidden activations stay in registers.  ``w_row``: per layer the weights packed with one
    column block (pack_node_layer(..)["w_row"]), ``bias`` / ``relu`` per layer.  Bit for bit the separate launches.
    The FIRST layer may contract over ``k_in0`` != width columns (320 -> 256), add ``mid_residual`` and store its fp32 result in
    ``mid_out_f32`` (which may be the last layer's ``residual``); ``mid_ln`` = (gamma, beta, eps): a LayerNorm of the first layer behind
    that residual (an encoder layer's out_proj + residual + norm1 in front of its feed-forward).  -> (out_f32, out_xp) like ``node_linear``."""
    lib = load_library()
    _req(xp, torch.int16, "xp")
    n = len(w_row)
    mg, mb, meps = mid_ln if mid_ln is not None else (None, None, 0.0)
    k0 = width if k_in0 is None or k_in0 < 0 else int(k_in0)
    if n not in (2, 3, 4) or len(bias) != n or len(relu) != n or width not in CHAIN_WIDTHS or (k0 != width and (width, k0) != (256, 320)):
        raise HipLibraryError("node_chain: 2 .. 4 layers of width 256 or 320 (first layer: 320 -> 256 allowed)")
    dev = xp.device
    arr = (_ChainLayer * n)()
    for i in range(n):
        _req(w_row[i], torch.int16, "w_row"); _req(bias[i], name="bias")
        if w_row[i].numel() != width * (k0 if i == 0 else width) * 2 or bias[i].numel() < width:
            raise HipLibraryError("node_chain: weights must be packed with one column block of the layer's width")
        arr[i].w_packed, arr[i].bias, arr[i].relu = w_row[i].data_ptr(), bias[i].data_ptr(), int(bool(relu[i]))
    for nme, t in (("pre_mask", pre_mask), ("residual", residual), ("ln_gamma", ln_gamma), ("ln_beta", ln_beta), ("post_mask", post_mask),
                   ("mid_residual", mid_residual), ("mid_out_f32", mid_out_f32), ("mid_ln.gamma", mg), ("mid_ln.beta", mb)):
        if t is not None:
            _req(t, name=nme)
    if out_f32 is None and want_f32:
        out_f32 = torch.empty(n_rows, width, device=dev, dtype=torch.float32)
    if out_xp is None and want_xp:
        out_xp_k = width if out_xp_k is None else out_xp_k
        out_xp = xp_alloc(n_rows, out_xp_k, dev)
    if out_xp is not None:
        out_xp_k = width if out_xp_k is None else out_xp_k
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_chain(
        _p(xp), ctypes.byref(arr), n, n_rows, width, k0, _p(mid_residual), mid_residual.shape[-1] if mid_residual is not None else 0,
        _p(mid_out_f32), mid_out_f32.shape[-1] if mid_out_f32 is not None else 0, _p(mg), _p(mb), float(meps), _p(pre_mask), _p(residual), residual.shape[-1] if residual is not None else 0,
        _p(ln_gamma), _p(ln_beta), float(ln_eps), _p(post_mask), _p(out_f32), out_f32.shape[-1] if out_f32 is not None else 0, out_col0,
        _p(out_xp), (out_xp_k or 0) // 16, out_xp_k0 // 16, _p(range_flag()), _stream()), flops=2 * n_rows * width * (k0 + (n - 1) * width)),
        "s2s_node_chain")
    return out_f32, out_xp


def node_apply_chain(x, layers, n_rows: int, relu, **kw):
    """``node_apply`` for a chain of square layers: ONE launch (s2s_node_chain) for packed-plane activations of a supported width,
    the layers one after the other otherwise (fp32 activations of the "f32" arithmetic; other widths).  ``relu``: per layer;
    ``kw``: the LAST layer's epilogue / outputs as for ``node_apply`` (residual, ln, pre_mask, post_mask, out_*, want_*)."""
    width = layers[0]["n"]
    first_res, first_out, first_ln = kw.pop("first_residual", None), kw.pop("first_out_f32", None), kw.pop("first_ln", None)
    k0 = layers[0]["k"]
    ok = (x.dtype == torch.int16 and len(layers) in (2, 3, 4) and width in CHAIN_WIDTHS and (k0 == width or (width, k0) == (256, 320))
          and all(L["n"] == width for L in layers) and all(L["k"] == width for L in layers[1:])
          and "pre_scale" not in kw and "row_map" not in kw)
    # 320-wide chains (10 tiles: 512 registers, one workgroup per CU) win only between ~64 and ~384 workgroups: below, the first layer
    # is faster in narrow column blocks; above, two co-resident workgroups of the single launches overlap (tools/node_chain_bench.py:
    # 2 x 320: 38 -> 47 us at 1260 rows, 78 -> 70 at 32768, 182 -> 194 at 80000; 3 x 256: 55 -> 44, 74 -> 63, 201 -> 176)
    if ok and width == 320 and not (64 <= (n_rows + 127) // 128 <= 384):
        ok = False
    if not ok:
        act = x
        for i, L in enumerate(layers[:-1]):
            fk = dict(residual=first_res, out_f32=first_out, want_f32=first_out is not None, ln=first_ln) if i == 0 else dict(want_f32=False)
            _, act = node_apply(act, L, n_rows, relu=relu[i], want_xp=True, **fk)
        return node_apply(act, layers[-1], n_rows, relu=relu[-1], **kw)
    kw = dict(kw)
    ln = kw.pop("ln", None)
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    return torch.ops.str2str_amd.node_chain(x, [L["w_row"] for L in layers], [L["b"] for L in layers], [bool(r) for r in relu], n_rows, width,
                                            kw.pop("pre_mask", None), kw.pop("residual", None), g, b, float(eps), kw.pop("post_mask", None),
                                            kw.pop("out_f32", None), kw.pop("out_col0", 0), kw.pop("want_f32", True), kw.pop("out_xp", None),
                                            -1 if kw.get("out_xp_k") is None else kw.pop("out_xp_k"), kw.pop("out_xp_k0", 0),
                                            kw.pop("want_xp", False), k0, first_res, first_out,
                                            *(first_ln if first_ln is not None else (None, None, 0.0)))


_CONST_ROWS = {}


def const_rows(n_rows: int, value: float, device) -> torch.Tensor:
    """A cached [n_rows] float32 device tensor of ``value`` (a constant ``pre_scale`` of a node layer)."""
    key = (int(n_rows), float(value), str(device))
    t = _CONST_ROWS.get(key)
    if t is None:
        if len(_CONST_ROWS) > 64:
            _CONST_ROWS.clear()
        t = _CONST_ROWS[key] = torch.full((n_rows,), float(value), device=device, dtype=torch.float32)
    return t


def node_apply_multi(x, specs, n_rows: int):
    """Several layers of ONE input in one launch: ``specs`` = [(layer, kwargs)], kwargs as for ``node_apply`` restricted to what the
    multi-problem kernel carries (relu, pre_scale, out_f32 / out_col0 / want_f32, out_xp / out_xp_k / out_xp_k0 / want_xp).
    -> [(out_f32, out_xp)] like ``node_apply``.  fp32 activations (arithmetic "f32") run the layers one after the other."""
    if x.dtype != torch.int16 or len(specs) > 6 or len(specs) < 2:
        return [node_apply(x, layer, n_rows, **kw) for layer, kw in specs]
    dev = x.device
    empty_f, empty_i = torch.empty(0, device=dev), torch.empty(0, dtype=torch.int16, device=dev)
    w, bias, ps, dims, of, ox, res = [], [], [], [], [], [], []
    for layer, kw in specs:
        if set(kw) - {"relu", "pre_scale", "out_f32", "out_col0", "want_f32", "out_xp", "out_xp_k", "out_xp_k0", "want_xp"}:
            raise HipLibraryError(f"node_apply_multi: unsupported epilogue option in {sorted(kw)}")
        key, tg = small_rows_variant(layer, n_rows)
        o32, oxp = kw.get("out_f32"), kw.get("out_xp")
        if o32 is None and kw.get("want_f32", True):
            o32 = torch.empty(n_rows, layer["n"], device=dev, dtype=torch.float32)
        xk = kw.get("out_xp_k")
        if oxp is None and kw.get("want_xp", False):
            xk = layer["n"] if xk is None else xk
            oxp = xp_alloc(n_rows, xk, dev)
        if oxp is not None and xk is None:
            xk = layer["n"]
        w.append(layer[key]); bias.append(layer["b"]); ps.append(kw["pre_scale"] if kw.get("pre_scale") is not None else empty_f)
        dims += [n_rows, layer["k"], layer["n"], tg, o32.shape[-1] if o32 is not None else 0, kw.get("out_col0", 0), xk or 0,
                 kw.get("out_xp_k0", 0), int(bool(kw.get("relu", False)))]
        of.append(o32 if o32 is not None else empty_f); ox.append(oxp if oxp is not None else empty_i)
        res.append((o32, oxp))
    torch.ops.str2str_amd.node_linear_multi(x, w, bias, ps, dims, of, ox)
    return res


def encoder_attention(qkv: torch.Tensor, key_bias: Optional[torch.Tensor], n_samples: int, n_res: int, n_heads: int = 4,
                      want_f32: bool = False, want_xp: bool = True, arith: str = "f32"):
    """Self-attention core of one encoder layer on the in_proj output qkv [B*N, 3*D] -> (fp32 [B*N, D] or None, packed planes or
    None).  ``key_bias`` [B,N] is added to the logits of key j (None = zeros).  ``arith``: "f32" = exact fp32 MFMA, "f16x3" = split-f16
    MFMA (str2str_amd/arith.py)."""
    lib = load_library()
    _req(qkv, name="qkv")
    M, D3 = qkv.shape
    D = D3 // 3
    if M != n_samples * n_res or D % n_heads:
        raise HipLibraryError("encoder_attention: bad shapes")
    if key_bias is not None:
        _req(key_bias, name="key_bias")
    out = torch.empty(M, D, device=qkv.device, dtype=torch.float32) if want_f32 else None
    oxp = xp_alloc(M, D, qkv.device) if want_xp else None
    if arith not in ("f32", "f16x3"):
        raise HipLibraryError(f"encoder_attention: arith {arith!r}")
    fn = lib.s2s_encoder_attention_f16x3 if arith == "f16x3" else lib.s2s_encoder_attention
    rw = _p(range_flag()) if want_xp or arith == "f16x3" else None   # (the fp32 kernel splits only what it writes to out_xp)
    _check(_timed("s2s_encoder_attention", lambda: fn(_p(qkv), _p(key_bias), _p(out), _p(oxp), n_samples, n_res, n_heads, D // n_heads,
                                                      rw, _stream())), "s2s_encoder_attention")
    return out, oxp


def ca_sample_stats(ca: torch.Tensor, clash_bar: float = 3.0, k_exclusion: int = 0):
    """CA [R, L, 3] fp32 device tensor -> (n_clash [R] int32, adjacent_max [R] fp32, radius_of_gyration [R] fp64)."""
    lib = load_library()
    _req(ca, name="ca")
    R, L = ca.shape[:2]
    nc = torch.empty(R, dtype=torch.int32, device=ca.device)
    am = torch.empty(R, dtype=torch.float32, device=ca.device)
    rg = torch.empty(R, dtype=torch.float64, device=ca.device)
    _check(lib.s2s_ca_sample_stats(_p(ca), R, L, float(clash_bar), int(k_exclusion), _p(nc), _p(am), _p(rg), _stream()), "s2s_ca_sample_stats")
    return nc, am, rg


def ca_pairwise_distances(ca: torch.Tensor, offset: int = 1) -> torch.Tensor:
    """Upper-triangular CA distances [R, D] float32 of every sample (np.triu_indices(L, k=offset) order) in numpy's float32 arithmetic."""
    lib = load_library()
    _req(ca, name="ca")
    R, L = ca.shape[0], ca.shape[1]
    if ca.ndim != 3 or ca.shape[2] != 3 or L <= offset:
        raise HipLibraryError(f"ca_pairwise_distances: coordinates {tuple(ca.shape)}, offset {offset}")
    D = (L - offset) * (L - offset + 1) // 2
    out = torch.empty(R, D, dtype=torch.float32, device=ca.device)
    for r0 in range(0, R, 65535):
        n = min(65535, R - r0)
        _check(lib.s2s_ca_pairwise_distances(_p(ca[r0:r0 + n]), n, L, int(offset), _p(out[r0:r0 + n]), _stream()), "s2s_ca_pairwise_distances")
    return out


def ca_pwd_js(ref_ca: torch.Tensor, pred_ca: torch.Tensor, offset: int = 3, n_bins: int = 50, pseudo: float = 1e-6,
              ref_weights: Optional[torch.Tensor] = None, pred_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per pair channel Jensen-Shannon distance between the distance histograms of two CA ensembles -> [D] fp64.
    ``ref_weights`` / ``pred_weights``: per-sample float64 histogram weights (device tensors), None = ones."""
    lib = load_library()
    _req(ref_ca, name="ref_ca"); _req(pred_ca, name="pred_ca")
    L = ref_ca.shape[1]
    if pred_ca.shape[1] != L:
        raise HipLibraryError("ca_pwd_js: the ensembles have different lengths")
    for nme, w, n in (("ref_weights", ref_weights, ref_ca.shape[0]), ("pred_weights", pred_weights, pred_ca.shape[0])):
        if w is not None:
            _req(w, torch.float64, nme)
            if w.numel() != n:
                raise HipLibraryError(f"ca_pwd_js: {nme} has {w.numel()} entries for {n} samples")
    out = torch.empty((L - offset) * (L - offset + 1) // 2, dtype=torch.float64, device=ref_ca.device)
    _check(lib.s2s_ca_pwd_js(_p(ref_ca), ref_ca.shape[0], _p(pred_ca), pred_ca.shape[0], L, int(offset), int(n_bins), float(pseudo),
                             _p(out), _p(ref_weights), _p(pred_weights), _stream()), "s2s_ca_pwd_js")
    return out


def _rmsd_weights(weights, L: int, device):
    if weights is None:
        return None
    w = torch.as_tensor(weights).to(device, torch.float32).contiguous()
    if w.shape != (L,):
        raise HipLibraryError(f"weights: expected [{L}] (one per residue), got {tuple(w.shape)}")
    return w


RMSD_LAUNCH_PAIRS = 2 ** 31 - 1   # s2s_ca_rmsd_matrix takes fewer than 2^31 pairs per call


def rmsd_row_chunk(n_b: int, max_pairs: Optional[int] = None) -> int:
    """Rows of A per s2s_ca_rmsd_matrix call so that one call stays within ``max_pairs`` pairs (at least one row)."""
    cap = RMSD_LAUNCH_PAIRS if max_pairs is None else min(int(max_pairs), RMSD_LAUNCH_PAIRS)
    return max(1, min(cap // n_b, 16 * 65535))


def ca_rmsd_matrix(a: torch.Tensor, b: Optional[torch.Tensor] = None, weights=None, max_pairs: Optional[int] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Minimum RMSD (optimal proper rotation + translation, float64) of every pair of a [Ra, L, 3] and b [Rb, L, 3] fp32 device tensors
    -> [Ra, Rb] fp64.  ``b=None``: the self matrix of ``a`` (exactly symmetric).  ``weights``: per-residue [L], >= 0.  ``max_pairs``
    bounds the pairs (and with them the scratch) of one launch: rows are chunked, the result is bit for bit the same for any value.
    The caller bounds Ra x Rb (the output); metrics.coverage_rmsd shows the chunked use that never holds the whole matrix."""
    lib = load_library()
    _req(a, name="a")
    b = a if b is None else _req(b, name="b")
    if a.ndim != 3 or b.ndim != 3 or a.shape[2] != 3 or b.shape[1:] != a.shape[1:] or a.shape[0] < 1 or b.shape[0] < 1 or a.shape[1] < 1:
        raise HipLibraryError(f"ca_rmsd_matrix: coordinates {tuple(a.shape)} and {tuple(b.shape)}")
    (n_a, L), n_b = a.shape[:2], b.shape[0]
    w = _rmsd_weights(weights, L, a.device)
    if out is None:
        out = torch.empty(n_a, n_b, dtype=torch.float64, device=a.device)
    rows = rmsd_row_chunk(n_b, max_pairs)
    region = lambda n: -(-n // 16) * 16 * (3 * (-(-L // 4) * 4) + 1)  # noqa: E731
    ws = torch.empty(2 + region(n_b) + region(min(rows, n_a)), dtype=torch.float64, device=a.device)
    for r0 in range(0, n_a, rows):
        n = min(rows, n_a - r0)
        _check(lib.s2s_ca_rmsd_matrix(_p(a[r0:r0 + n]), n, _p(b), n_b, L, _p(w), _p(out[r0:r0 + n]), _p(ws), ws.numel(), _stream()),
               "s2s_ca_rmsd_matrix")
    return out


def ca_superpose(mobile: torch.Tensor, target: torch.Tensor, weights=None):
    """mobile [R, L, 3] onto target [L, 3] (fp32 device tensors) -> (rmsd [R] fp64, xform [R, 12] fp64: row-major proper rotation, then
    translation; rotation @ x + translation maps mobile onto target)."""
    lib = load_library()
    _req(mobile, name="mobile"); _req(target, name="target")
    if mobile.ndim != 3 or mobile.shape[2] != 3 or target.shape != mobile.shape[1:] or mobile.shape[0] < 1 or mobile.shape[1] < 1:
        raise HipLibraryError(f"ca_superpose: mobile {tuple(mobile.shape)}, target {tuple(target.shape)}")
    R, L = mobile.shape[:2]
    w = _rmsd_weights(weights, L, mobile.device)
    rmsd = torch.empty(R, dtype=torch.float64, device=mobile.device)
    xform = torch.empty(R, 12, dtype=torch.float64, device=mobile.device)
    _check(lib.s2s_ca_superpose(_p(mobile), R, _p(target), L, _p(w), _p(rmsd), _p(xform), _stream()), "s2s_ca_superpose")
    return rmsd, xform


def apply_xform(points: torch.Tensor, xform: torch.Tensor) -> torch.Tensor:
    """points [R, M, 3] fp32, xform [R, 12] fp64 (ca_superpose) -> rotation @ point + translation, float64 arithmetic, fp32 result."""
    lib = load_library()
    _req(points, name="points"); _req(xform, torch.float64, "xform")
    if points.ndim != 3 or points.shape[2] != 3 or xform.shape != (points.shape[0], 12) or points.shape[0] < 1 or points.shape[1] < 1:
        raise HipLibraryError(f"apply_xform: points {tuple(points.shape)}, xform {tuple(xform.shape)}")
    out = torch.empty_like(points)
    _check(lib.s2s_apply_xform(_p(points), _p(xform), points.shape[0], points.shape[1], _p(out), _stream()), "s2s_apply_xform")
    return out


def unpack_planes(xp: torch.Tensor, n_rows: int, k: int) -> torch.Tensor:
    """XP -> fp32 [n_rows, k] (x_h + x_l of the f16 pair planes; for tests and debugging)."""
    KS = k // 16
    fr = xp.view(torch.float16).reshape(-1, KS, 2, 2, 32, 8).float().sum(2)    # [RT, KS, g, m, j]
    ks = torch.arange(KS)[:, None, None]
    g = torch.arange(2)[None, :, None]
    j = torch.arange(8)[None, None, :]
    r = 8 * (ks & 1) + j
    chan = (32 * (ks >> 1) + (r & 3) + 8 * (r >> 2) + 4 * g).to(xp.device)     # [KS, 2, 8]
    out = torch.zeros(fr.shape[0], 32, k, device=xp.device)
    out[:, :, chan.reshape(-1)] = fr.permute(0, 3, 1, 2, 4).reshape(fr.shape[0], 32, -1)
    return out.reshape(-1, k)[:n_rows]


# ------------------------------------------------------------------------------------------ PDB text (host side of the ABI)
def _np_or_none(x, dtype):
    if x is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(x), dtype=dtype)
    return a, a.ctypes.data_as(_vp)


def _pdb_args(atom37, aatype, residue_index, chain_index, b_factors):
    pos = np.ascontiguousarray(np.asarray(atom37), dtype=np.float32)
    if pos.ndim == 3:
        pos = pos[None]
    if pos.ndim != 4 or pos.shape[-2:] != (37, 3):
        raise ValueError(f"Invalid positions shape {pos.shape}")
    n = pos.shape[1]
    sq = lambda x: None if x is None else (np.squeeze(np.asarray(x)) if np.asarray(x).shape[0] == 1 and np.asarray(x).ndim > 1 else np.asarray(x))  # noqa: E731
    keep = [pos]
    ptrs = [pos.ctypes.data_as(_vp), pos.shape[0], n]
    for x, dt, want in ((aatype, np.int64, (n,)), (residue_index, np.int64, (n,)), (chain_index, np.int64, (n,)),
                        (b_factors, np.float64, (n, 37))):
        a, p = _np_or_none(sq(x), dt)
        if a is not None and a.shape != want:
            raise ValueError(f"expected shape {want}, got {a.shape}")
        keep.append(a)
        ptrs.append(p)
    return keep, ptrs


def _pdb_rc(rc, what):
    if rc == -1:
        raise ValueError("Invalid aatypes." if what != "merge" else "bad arguments")
    if rc == -2:
        raise ValueError("The PDB format supports at most 62 chains.")
    if rc < 0:
        raise OSError(f"{what}: I/O error {rc}")
    return rc


def format_pdb_models(atom37, aatype=None, residue_index=None, chain_index=None, b_factors=None, first_model: int = 1,
                      add_end: int = 2) -> str:
    """Text of ``atom37_to_pdb`` (add_end=2) / ``to_pdb`` per model (add_end=1 / 0) for atom37 [M,N,37,3] or [N,37,3]."""
    lib = load_library()
    keep, a = _pdb_args(atom37, aatype, residue_index, chain_index, b_factors)
    need = _pdb_rc(lib.s2s_format_pdb_models(*a, int(first_model), int(add_end), None, 0), "format")
    buf = ctypes.create_string_buffer(int(need) + 1)
    got = _pdb_rc(lib.s2s_format_pdb_models(*a, int(first_model), int(add_end), ctypes.cast(buf, _vp), int(need)), "format")
    assert got == need
    return buf.raw[:need].decode("ascii")


def write_pdb_models(path: str, atom37, aatype=None, residue_index=None, chain_index=None, b_factors=None,
                     first_model: int = 1, add_end: int = 2, append: bool = False) -> int:
    """Stream the same text to ``path`` (bounded memory); returns the number of bytes written."""
    lib = load_library()
    keep, a = _pdb_args(atom37, aatype, residue_index, chain_index, b_factors)
    return _pdb_rc(lib.s2s_write_pdb_models(os.fsencode(path), int(bool(append)), *a, int(first_model), int(add_end)), "write")


def merge_pdb_files(paths, out_path: str) -> int:
    lib = load_library()
    enc = [os.fsencode(p) for p in paths]
    arr = (ctypes.c_char_p * len(enc))(*enc)
    return _pdb_rc(lib.s2s_merge_pdb_files(ctypes.cast(arr, _vp), len(enc), os.fsencode(out_path)), "merge")


# ------------------------------------------------------------------------------------------ host noise stream (parity mode)
_HOST_RNG_OK = None   # None: not checked yet; True / False: the fast-forward reproduces torch's own draws on this build (or not)
_ST_LEFT, _ST_NEXT, _ST_WORDS, _ST_END = 8, 16, 24, 24 + 624 * 8   # byte offsets in torch.get_rng_state(): seed u64 | left i32 | seeded i32 | next u64 | 624 x u64


def float64_normal_outputs(n_elements: int) -> int:
    """32-bit engine outputs one float64 ``torch.randn`` of ``n_elements`` >= 16 consumes (ATen normal_fill: n uniform doubles of two
    outputs each, and the last block of 16 once more when n is not a multiple of 16)."""
    return 2 * (n_elements + (16 if n_elements % 16 else 0))


def _host_rng_discard_raw(n_outputs: int) -> bool:
    st = torch.get_rng_state()
    if st.numel() < _ST_END or st.dtype != torch.uint8:
        return False
    buf = st.numpy()          # (shares memory with st)
    left = ctypes.c_int(int(np.frombuffer(buf, np.int32, 1, _ST_LEFT)[0]))
    nxt = ctypes.c_ulonglong(int(np.frombuffer(buf, np.uint64, 1, _ST_NEXT)[0]))
    words = np.frombuffer(buf, np.uint64, 624, _ST_WORDS)
    if load_library().s2s_mt19937_discard(words.ctypes.data, ctypes.byref(left), ctypes.byref(nxt), ctypes.c_ulonglong(int(n_outputs))) != 0:
        return False
    np.frombuffer(buf, np.int32, 1, _ST_LEFT)[0] = left.value
    np.frombuffer(buf, np.uint64, 1, _ST_NEXT)[0] = nxt.value
    torch.set_rng_state(st)
    return True


def host_rng_fast_forward_ok() -> bool:
    """Does ``host_rng_discard`` leave torch's CPU generator exactly where real float64 normal draws leave it?  Checked ONCE per process
    against the draws themselves (sizes with and without the re-drawn tail block, across several twists of the engine); the
    generator is left as it was found.  False (layout of another torch build, no library) -> callers draw for real."""
    global _HOST_RNG_OK
    if _HOST_RNG_OK is None:
        keep = torch.get_rng_state()
        try:
            ok = True
            for seed, sizes in ((1234567, (48, 50, 4800, 17)), (7, (15360, 3780, 3780, 16))):
                torch.default_generator.manual_seed(seed)       # the CPU generator ONLY (torch.manual_seed would reseed every device generator too)
                torch.rand(3)                                   # an engine position that is not a block boundary
                start = torch.get_rng_state()
                for n in sizes:
                    torch.randn(n, dtype=torch.float64)
                want, probe = torch.get_rng_state(), torch.rand(4)
                torch.set_rng_state(start)
                ok = ok and _host_rng_discard_raw(sum(float64_normal_outputs(n) for n in sizes))
                ok = ok and torch.equal(torch.get_rng_state(), want) and torch.equal(torch.rand(4), probe)
            _HOST_RNG_OK = bool(ok)
        except Exception:
            _HOST_RNG_OK = False
        finally:
            torch.set_rng_state(keep)
    return _HOST_RNG_OK


def host_rng_can_discard(n_elements: int) -> bool:
    """Would ``host_rng_discard_float64_normals`` fast-forward over float64 normal tensors of ``n_elements`` elements here?"""
    return n_elements >= 16 and os.environ.get("S2S_HOST_RNG_FAST", "1") != "0" and host_rng_fast_forward_ok()


def host_rng_discard_float64_normals(n_elements: int, n_tensors: int) -> bool:
    """Advance torch's CPU generator as ``n_tensors`` draws ``torch.randn(n_elements, dtype=float64)`` would, without computing them
    (s2s_mt19937_discard).  -> False if that is not possible here (tensors below 16 elements take ATen's scalar path; an unknown state
    layout): the caller draws for real."""
    if n_tensors <= 0:
        return True
    if not host_rng_can_discard(n_elements):
        return False
    return _host_rng_discard_raw(float64_normal_outputs(n_elements) * int(n_tensors))


_registered = False


def _ln3(g, b, eps):
    return None if g is None else (g, b, eps)


def _opt_int(v):
    return None if v is None or v < 0 else v


# (the dispatcher passes positional arguments up to the last one the caller gave: the implementations carry the schema's defaults)
def _op_node_linear(xp, wpk, bias, n_rows, k_in, n_out, tiles, pre_scale=None, relu=False, pre_mask=None, residual=None, ln_gamma=None,
                    ln_beta=None, ln_eps=0.0, post_mask=None, out_f32=None, out_col0=0, want_f32=True, out_xp=None, out_xp_k=-1,
                    out_xp_k0=0, want_xp=False, map_pad=0, map_src=0):
    return node_linear(xp, wpk, bias, n_rows, k_in, n_out, tiles, pre_scale=pre_scale, relu=relu, pre_mask=pre_mask, residual=residual,
                       ln=_ln3(ln_gamma, ln_beta, ln_eps), post_mask=post_mask, out_f32=out_f32, out_col0=out_col0, want_f32=want_f32,
                       out_xp=out_xp, out_xp_k=_opt_int(out_xp_k), out_xp_k0=out_xp_k0, want_xp=want_xp,
                       row_map=(map_pad, map_src) if map_pad else None)


def _op_node_linear_f32(x, wpk32, bias, n_rows, k_in, n_out, tiles, pre_scale=None, relu=False, pre_mask=None, residual=None, ln_gamma=None,
                        ln_beta=None, ln_eps=0.0, post_mask=None, out=None, out_col0=0):
    return node_linear_f32(x, wpk32, bias, n_rows, k_in, n_out, tiles, pre_scale=pre_scale, relu=relu, pre_mask=pre_mask,
                           residual=residual, ln=_ln3(ln_gamma, ln_beta, ln_eps), post_mask=post_mask, out=out, out_col0=out_col0)


def _op_edge_transition_f16x3_chain(edge, in_tiled, B, N, node_ab, node_p, wstream, b2, gamma, beta, mask, ln_eps, proj_bias64,
                                    out_layout, prescale_exp=0, ab_kernel_form=False):
    """The trunk's form of the edge transition: pair tensor in either layout (``edge`` = the flat tiled buffer when ``in_tiled``), the
    next IPA block's projections fused in when ``proj_bias64`` is given (``wstream`` is then the 31-stage stream).
    -> (pair tensor (row-major [B,N,N,128] | flat tiled buffer | None), attn_bias | None, pair_z | None)"""
    e = PairTiled(B, N, buf=edge) if in_tiled else edge
    r = edge_transition_f16x3(e, node_ab, node_p, wstream, b2, gamma, beta, mask, ln_eps,
                              proj=None if proj_bias64 is None else (wstream, proj_bias64), out_layout=out_layout, prescale_exp=prescale_exp,
                              ab_kernel_form=ab_kernel_form)
    z, bias, pz = r if proj_bias64 is not None else (r, None, None)
    return (z.buf if isinstance(z, PairTiled) else z), bias, pz


_TORCH_OPS = {
    # ---- pair stream
    "edge_transition(Tensor edge, Tensor node_ab, Tensor node_p, Tensor w1p, Tensor w2p, Tensor wfp, Tensor b2, "
    "Tensor bf, Tensor gamma, Tensor beta, Tensor? mask, float ln_eps) -> Tensor": lambda *a: edge_transition(*a),
    "edge_transition_f16x3(Tensor edge, Tensor node_ab, Tensor node_p, Tensor wstream, Tensor b2, "
    "Tensor gamma, Tensor beta, Tensor? mask, float ln_eps, int prescale_exp=0) -> Tensor":
        lambda e, nab, np_, ws, b2, g, b, m, eps, pe=0: edge_transition_f16x3(e, nab, np_, ws, b2, g, b, m, eps, prescale_exp=pe),
    "edge_transition_f16x3_chain(Tensor edge, bool in_tiled, int B, int N, Tensor node_ab, Tensor node_p, Tensor wstream, Tensor b2, "
    "Tensor gamma, Tensor beta, Tensor? mask, float ln_eps, Tensor? proj_bias64, str out_layout, int prescale_exp=0, "
    "bool ab_kernel_form=False) "
    "-> (Tensor?, Tensor?, Tensor?)":
        _op_edge_transition_f16x3_chain,
    "edge_embed(Tensor node_a, Tensor node_b, Tensor rel_table, Tensor bin_table, Tensor bin_lower, Tensor residue_idx, Tensor ca, "
    "Tensor w2p, Tensor w3p, Tensor b2, Tensor b3, Tensor gamma, Tensor beta, Tensor? mask, int rel_offset, float ln_eps) -> Tensor":
        lambda *a: edge_embed(*a),
    "edge_embed_f16x3(Tensor node_a, Tensor node_b, Tensor rel_table, Tensor bin_table, Tensor bin_lower, "
    "Tensor residue_idx, Tensor ca, Tensor wstream, Tensor b2, Tensor b3, Tensor gamma, Tensor beta, Tensor? mask, "
    "int rel_offset, float ln_eps) -> Tensor": lambda *a: edge_embed_f16x3(*a),
    "pair_project(Tensor edge, Tensor wp, Tensor bias64) -> (Tensor, Tensor)": lambda *a: pair_project(*a),
    # ---- attention
    "ipa_prep_points(Tensor rigids7, Tensor q_pts_lin, Tensor kv_pts_lin, int n_heads=8, int n_qk=8, int n_v=12) -> (Tensor, Tensor, Tensor)":
        lambda *a: ipa_prep_points(*a),
    "ipa_attention(Tensor q, Tensor kv, Tensor q_pts, Tensor k_pts, Tensor v_pts, Tensor attn_bias, Tensor pair_z, "
    "Tensor mask, Tensor rigids7, Tensor head_w) -> Tensor": lambda *a: ipa_attention(*a),
    "ipa_prep_points_f16(Tensor rigids7, Tensor q_pts_lin, Tensor kv_pts_lin, Tensor head_w, int n_heads=8, int n_qk=8, int n_v=12, "
    "int c_hidden=256) -> (Tensor, Tensor, Tensor, Tensor, Tensor)": lambda *a: ipa_prep_points_f16(*a),
    "ipa_prep_points_shared_kv(Tensor rigids7, Tensor q_pts_lin, Tensor kv_pts_lin, Tensor head_w, Tensor s_xp, int n_heads=8, int n_qk=8, "
    "int n_v=12, int c_hidden=256) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor?, Tensor)":
        lambda r7, qp, kvp, hw, s_xp, h=8, nq=8, nv=12, c=256: ipa_prep_points_f16(r7, qp, kvp, hw, h, nq, nv, c, s_xp),
    "ipa_attention_f16w(Tensor q_xp, Tensor k_xp, Tensor v_vf, Tensor qp_xp, Tensor kp_xp, Tensor vp_vf, Tensor q2, Tensor k2, "
    "Tensor(a!) attn_bias, Tensor pair_z, Tensor mask, Tensor rigids7, int n_heads=8, int c_hidden=256, int n_qk=8, int n_v=12, int c_pz=32, "
    "float inf=1e5, float eps=1e-8, bool logits_inplace=False) -> (Tensor, Tensor)":
        lambda q, k, v, qp, kp, vp, q2, k2, ab, pz, m, r7, *rest: ipa_attention_f16(q, k, v, (qp, kp, vp, q2, k2), ab, pz, m, r7, *rest),
    "encoder_attention(Tensor qkv, Tensor? key_bias, int n_samples, int n_res, int n_heads=4, bool want_f32=False, bool want_xp=True, "
    "str arith='f32') -> (Tensor?, Tensor?)": lambda *a: encoder_attention(*a),
    # ---- node stream
    "node_linear(Tensor xp, Tensor wpk, Tensor? bias, int n_rows, int k_in, int n_out, int tiles, Tensor? pre_scale=None, bool relu=False, "
    "Tensor? pre_mask=None, Tensor? residual=None, Tensor? ln_gamma=None, Tensor? ln_beta=None, float ln_eps=0.0, Tensor? post_mask=None, "
    "Tensor(a!)? out_f32=None, int out_col0=0, bool want_f32=True, Tensor(b!)? out_xp=None, int out_xp_k=-1, int out_xp_k0=0, "
    "bool want_xp=False, int map_pad=0, int map_src=0) -> (Tensor?, Tensor?)": _op_node_linear,
    "node_linear_f32(Tensor x, Tensor wpk32, Tensor? bias, int n_rows, int k_in, int n_out, int tiles, Tensor? pre_scale=None, "
    "bool relu=False, Tensor? pre_mask=None, Tensor? residual=None, Tensor? ln_gamma=None, Tensor? ln_beta=None, float ln_eps=0.0, "
    "Tensor? post_mask=None, Tensor(a!)? out=None, int out_col0=0) -> Tensor": _op_node_linear_f32,
    "node_linear_vfrag(Tensor xp, Tensor wpk, Tensor? bias, int n_rows, int k_in, int n_out, int tiles_per_head=8, int map_pad=0, "
    "int map_src=0) -> Tensor":
        lambda xp, w, b, m, k, n, tph=8, mp=0, ms=0: node_linear_vfrag(xp, w, b, m, k, n, tph, row_map=(mp, ms) if mp else None),
    "ipa_projections(Tensor s_xp, Tensor[] q, Tensor[] k, Tensor[] v, Tensor[] qp, Tensor[] kvp, int[] dims, int n_rows, int n_rows_padded, "
    "int map_pad=0, int map_src=0) -> (Tensor, Tensor?, Tensor?, Tensor, Tensor)":      # (k / v: empty lists = absent, folded projections)
        lambda s_xp, q, k, v, qp, kvp, dims, m, mo, mp=0, ms=0: ipa_projections(
            s_xp, *[({"w": t[0], "b": t[1], "k": dims[3 * i], "n": dims[3 * i + 1], "tg": dims[3 * i + 2]} if len(t) else None)
                    for i, t in enumerate((q, k, v, qp, kvp))],
            m, mo, (mp, ms) if mp else None),
    "embed_assemble(Tensor t_img, Tensor node_const, Tensor fa, Tensor fb, int n_samples, int n_res, bool planes, bool b_col_blocked) "
    "-> (Tensor, Tensor, Tensor)": lambda *a: embed_assemble(*a),
    "node_linear_multi(Tensor xp, Tensor[] w, Tensor[] bias, Tensor[] pre_scale, int[] dims, Tensor(a!)[] out_f32, Tensor(b!)[] out_xp) -> ()":
        lambda *a: node_linear_multi(*a),
    "node_chain(Tensor xp, Tensor[] w_row, Tensor[] bias, bool[] relu, int n_rows, int width, Tensor? pre_mask=None, Tensor? residual=None, "
    "Tensor? ln_gamma=None, Tensor? ln_beta=None, float ln_eps=0.0, Tensor? post_mask=None, Tensor(a!)? out_f32=None, int out_col0=0, "
    "bool want_f32=True, Tensor(b!)? out_xp=None, int out_xp_k=-1, int out_xp_k0=0, bool want_xp=False, int k_in0=-1, "
    "Tensor? mid_residual=None, Tensor(c!)? mid_out_f32=None, Tensor? mid_ln_gamma=None, Tensor? mid_ln_beta=None, float mid_ln_eps=0.0) "
    "-> (Tensor?, Tensor?)":
        lambda xp, w, b, r, m, wd, pm=None, res=None, g=None, be=None, eps=0.0, pom=None, of=None, oc=0, wf=True, ox=None, ok=-1, ok0=0, wx=False,
        k0=-1, mr=None, mo=None, mg=None, mb=None, me=0.0: node_chain(xp, w, b, r, m, wd, pm, res, g, be, eps, pom, of, oc, wf, ox, _opt_int(ok), ok0, wx,
                                                                      k0, mr, mo, (mg, mb, me) if mg is not None else None),
    "row_layernorm(Tensor x, int n_rows, int n_cols, Tensor gamma, Tensor beta, float eps, Tensor? post_mask=None, Tensor(a!)? out_f32=None, "
    "int out_col0=0, bool want_f32=True, Tensor(b!)? out_xp=None, int out_xp_k=-1, int out_xp_k0=0, bool want_xp=False) -> (Tensor?, Tensor?)":
        lambda x, m, n, g, b, eps, pm=None, of=None, oc=0, wf=True, ox=None, ok=-1, ok0=0, wx=False: row_layernorm(
            x, m, n, g, b, eps, pm, of, oc, wf, ox, _opt_int(ok), ok0, wx),
    "pack_planes(Tensor x, int col0=0, int n_cols=-1, Tensor(a!)? out=None, int out_k=-1, int k0=0, Tensor? row_scale=None) -> Tensor":
        lambda x, c0=0, nc=-1, out=None, ok=-1, k0=0, rs=None: pack_planes(x, c0, _opt_int(nc), out, _opt_int(ok), k0, rs),
    # ---- frames / diffusion geometry
    "se3_step(Tensor x0_7, Tensor xt_7, Tensor mask, Tensor diffuse_mask, Tensor params8, float dt) -> Tensor":
        lambda x0, xt, m, dm, p8, dt: se3_step(x0, xt, m, dm, p8, dt)[0],
    "forward_marginal(Tensor? rigids0_4x4, Tensor z_axis, Tensor u01, Tensor z_trans, Tensor cdf_rows, Tensor row_of_sample, "
    "Tensor omega_grid, Tensor? params2, Tensor? diffuse_mask=None, float coordinate_scaling=0.1) -> Tensor":
        lambda *a: forward_marginal(*a),
    "rigid_compose_update(Tensor rigids7, Tensor update6, Tensor mask) -> Tensor": lambda *a: rigid_compose_update(*a),
    "rigid_scale_trans(Tensor rigids7, float scale, bool divide=False) -> Tensor": lambda *a: rigid_scale_trans(*a),
    "torsion_head(Tensor u, int n_rows, bool normalize=True, float eps=1e-8, Tensor? gt_sin_cos=None, Tensor? fixed_mask=None) -> Tensor":
        lambda *a: torsion_head(*a),
    "frames_to_backbone(Tensor rigids7, Tensor psi, Tensor? aatype) -> Tensor": lambda r, p, a: frames_to_backbone(r, p, a)[0],
}


def register_torch_ops():
    """Expose every tensor entry point of the library as ``torch.ops.str2str_amd.<name>`` (CUDA/HIP dispatch key only).
    The model's modules reach their kernels through these ops (``node_apply``, ``encoder_attention``, the attention and
    edge-transition call sites below and in models/net): ``torch.ops.str2str_amd`` is the operator surface, this module its
    implementation over the C ABI.  Called once at import time (bottom of this module): defining the schemas needs no GPU and no
    library; the kernels behind them load the shared object on first use."""
    global _registered
    if _registered:
        return
    lib = torch.library.Library("str2str_amd", "DEF")
    impl = torch.library.Library("str2str_amd", "IMPL", "CUDA")
    for schema, fn in _TORCH_OPS.items():
        lib.define(schema)
        impl.impl(schema.split("(")[0], fn)
    register_torch_ops._libs = (lib, impl)  # keep alive
    _registered = True


register_torch_ops()
