"""Range guard of the f16x3 kernels: the per-device flag buffer every split-f16 launch is handed, and how to read it."""
import torch

from .binding import HipLibraryError

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
