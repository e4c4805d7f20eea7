"""Host side of the ABI: PDB text and the fast-forward of torch's CPU generator (parity mode)."""
import ctypes
import os

import numpy as np
import torch

from .binding import _vp, load_library


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
        a = None if x is None else np.ascontiguousarray(sq(x), dtype=dt)
        if a is not None and a.shape != want:
            raise ValueError(f"expected shape {want}, got {a.shape}")
        keep.append(a)
        ptrs.append(None if a is None else a.ctypes.data_as(_vp))
    return keep, ptrs


def _pdb_rc(rc, what):
    if rc == -1:
        raise ValueError("Invalid aatypes." if what != "merge" else "bad arguments")
    if rc == -2:
        raise ValueError("The PDB format supports at most 62 chains.")
    if rc < 0:
        raise OSError(f"{what}: I/O error {rc}")
    return rc


def format_pdb_models(atom37, aatype=None, residue_index=None, chain_index=None, b_factors=None, first_model: int = 1, add_end: int = 2) -> str:
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
# None: not checked yet; True / False: the fast-forward reproduces torch's own draws on this build (or not).  Rebound by
# host_rng_fast_forward_ok: read it through that function only.
_HOST_RNG_OK = None
# byte offsets in torch.get_rng_state(): seed u64 | left i32 | seeded i32 | next u64 | 624 x u64
_ST_LEFT, _ST_NEXT, _ST_WORDS, _ST_END = 8, 16, 24, 24 + 624 * 8


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
