"""The ctypes side of libstr2str_hip.so: the typed entry points, the library handle and the argument helpers every wrapper uses."""
import ctypes
import os
from typing import Optional

import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # str2str_amd/: where build.py links the library
LIB_PATH = os.environ.get("STR2STR_HIP_LIB") or os.path.join(_PKG, "libstr2str_hip.so")  # env override: A/B builds
ABI_VERSION = 40

_lib = None   # rebound by load_library: read it through that function only

_vp, _i, _f, _d, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong

_SIGNATURES = {
    "s2s_abi_version": [],
    "s2s_edge_transition": [_vp] * 12 + [_i, _i, _f, _vp, _vp, _vp, _vp, _vp],
    "s2s_edge_transition_f16x3": [_vp] * 9 + [_i, _i, _f, _i, _vp, _vp, _vp, _i, _vp, _vp],
    "s2s_edge_embed": [_vp] * 15 + [_i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp],
    "s2s_edge_embed_f16x3": [_vp] * 14 + [_i, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp],
    "s2s_edge_embed_classes_f16x3": [_vp] * 10 + [_i, _i, _i, _f, _vp, _vp, _vp],
    "s2s_edge_embed_expand": [_vp] * 8 + [_i, _vp, _vp, _i, _i, _i, _i, _i, _vp],
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
    "s2s_ca_tm_matrix": [_vp, _i, _vp, _i, _i, _d, _vp, _vp],
    "s2s_ca_tm_superpose": [_vp, _i, _vp, _i, _d, _vp, _vp, _vp],
    "s2s_ca_lddt_matrix": [_vp, _i, _vp, _i, _i, _d, _i, _vp, _vp, _ll, _vp],
    "s2s_ca_lddt_per_residue": [_vp, _i, _vp, _i, _d, _i, _vp, _vp, _vp, _ll, _vp],
    "s2s_ca_contact_map": [_vp, _i, _i, _d, _i, _vp, _vp, _vp, _vp],
    "s2s_ca_contact_stats": [_vp, _i, _i, _d, _i, _vp, _vp, _vp],
    "s2s_ca_native_contacts": [_vp, _i, _d, _i, _vp, _vp, _vp, _vp],
    "s2s_ca_native_q": [_vp, _i, _i, _vp, _vp, _i, _d, _d, _vp, _vp, _vp, _vp],
    "s2s_backbone_violations": [_vp, _i, _i, _vp, _vp, _vp, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "s2s_secondary_structure": [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "s2s_backbone_sasa": [_vp, _i, _i, _vp, _vp, _d, _vp, _i, _vp, _vp, _vp, _vp],
    "s2s_ca_scattering": [_vp, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp],
    "s2s_ca_aligned_mean": [_vp, _i, _i, _vp, _vp, _vp, _vp],
    "s2s_ca_covariance": [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _ll, _vp],
    "s2s_ca_project": [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp],
    "s2s_lagged_mean": [_vp, _i, _i, _i, _vp, _vp],
    "s2s_lagged_covariances": [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _ll, _vp],
    "s2s_feature_project": [_vp, _i, _i, _vp, _vp, _i, _vp, _vp],
    "s2s_cluster_adjacency": [_vp, _i, _i, _i, _d, _i, _vp, _vp, _vp],
    "s2s_cluster_gromos": [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "s2s_format_pdb_models": [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _ll],
    "s2s_write_pdb_models": [ctypes.c_char_p, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i],
    "s2s_merge_pdb_files": [_vp, _i, ctypes.c_char_p],
    "s2s_mt19937_discard": [_vp, _vp, _vp, ctypes.c_ulonglong],
}
_LL_RETURN = ("s2s_format_pdb_models", "s2s_write_pdb_models", "s2s_merge_pdb_files")
EXPORTS = tuple(_SIGNATURES)

# The kinetics family (include/str2str_kinetics.h): the same library, a prefix, a table and a version of its own.
KINETICS_ABI_VERSION = 1
_KINETICS_SIGNATURES = {
    "s2k_abi_version": [],
    "s2k_assign": [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "s2k_centre_update": [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _ll, _vp],
    "s2k_farthest_point": [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _ll, _vp],
    "s2k_transition_counts": [_vp, _i, _vp, _i, _i, _i, _vp, _vp],
}
KINETICS_EXPORTS = tuple(_KINETICS_SIGNATURES)


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

    def total_ms(self, name):
        torch.cuda.synchronize()
        ev = self.events[name]
        return sum(a.elapsed_time(b) for a, b in ev), len(ev)

    def mean_ms(self, name):
        total, n = self.total_ms(name)
        return (total / n if n else float("nan")), n


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
        raise HipLibraryError(f"{p} not found: the HIP kernels are not built. Run `python -m str2str_amd.build` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback for the sampling path.")
    lib = ctypes.CDLL(p)
    for name, args in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.argtypes = args
        fn.restype = ctypes.c_longlong if name in _LL_RETURN else ctypes.c_int
    for name, args in _KINETICS_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    v = lib.s2s_abi_version()
    if v != ABI_VERSION:
        raise HipLibraryError(f"libstr2str_hip.so ABI {v} != expected {ABI_VERSION}; rebuild")
    v = lib.s2k_abi_version()
    if v != KINETICS_ABI_VERSION:
        raise HipLibraryError(f"libstr2str_hip.so kinetics ABI {v} != expected {KINETICS_ABI_VERSION}; rebuild")
    if path is None:
        _lib = lib
    return lib


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


def _req_all(dtype=torch.float32, /, **tensors):
    """``_req`` for several tensors of one dtype, each under its argument's name."""
    for name, t in tensors.items():
        _req(t, dtype, name)


def _req_opt(dtype=torch.float32, /, **tensors):
    """``_req_all`` for the optional arguments: a tensor the caller left out (None) is skipped."""
    _req_all(dtype, **{name: t for name, t in tensors.items() if t is not None})


# An optional int crosses the torch-op schemas as -1 (the dispatcher needs an int): callers encode with ``_int_arg``, the adapters in
# torch_ops.py decode with ``_opt_int``.
def _int_arg(v: Optional[int]) -> int:
    return -1 if v is None else v


def _opt_int(v: Optional[int]) -> Optional[int]:
    return None if v is None or v < 0 else v
