"""Guard bands and poisoned buffers for everything the ``ops`` wrappers allocate, and a recording proxy for the library handle.
A helper, not a conftest: tests/test_abi_bounds.py (device) and tests/test_guarded_alloc_cpu.py (the helper itself, on the CPU) import it.

``guarded(poison)`` replaces, for its duration, the tensor factories the wrappers use -- torch.empty / empty_like / zeros / zeros_like /
full and Tensor.new_empty / new_zeros / new_full -- by versions that carve the tensor out of a flat uint8 buffer of nbytes + 2 BAND:

    [ BAND bytes of 0xA5 | interior: poison (empty) or zeros / the fill value (zeros, full) | BAND bytes of 0xA5 ]

and return the interior viewed as the requested dtype and shape, contiguous.  A kernel that stores past either end of its buffer lands
in a band (``check_bands``) instead of in a neighbouring tensor; a kernel that leaves part of its output unwritten, accumulates into a
workspace it never cleared, or reads padding it should not, gives results that differ between the two poisons and from a plain call.
The bands see stores of up to BAND bytes past an end; a wilder store is outside what this helper can show.

``RecordingLib`` wraps the ctypes handle of libstr2str_hip.so: every ``s2s_*`` call is forwarded, and its name and the address of every
pointer argument (the descriptor arrays' pointer fields included) are recorded.  ``unaccounted`` then names every pointer that is
neither NULL, nor inside a guarded allocation, nor inside a tensor the test declared, nor the stream handle, nor listed as a host-side
argument: a buffer that reached a kernel by a route the guard does not replace is reported, not silently left unguarded.
"""
import contextlib
import ctypes
import math
import sys

import torch

# The widest unit any kernel of the library stores at once is a 32-pair x 128-float tile of the tiled pair layout: 32 * 128 * 4 B =
# 16 KiB.  The band is four times that, so a whole stray tile -- or four of them -- still lands inside memory the guard owns.
# A multiple of 512 bytes: the interior is then as aligned as a fresh allocation of the caching allocator.
BAND = 64 * 1024
BAND_BYTE = 0xA5

# Poison of an ``empty`` interior, as a byte, by dtype class.  Run A: 0xFF everywhere = NaN in f16, f32 and f64, -1 in the integers.
# Run B: 0x7B in the floating types and the int16 f16 planes = finite and huge (1.3e36 in f32, 61280 in f16 -- beyond the range
# guard's 2^15 --, 1e286 in f64), 0 in int32 / int64 / uint8: an uninitialised integer used as an index then stays next to its own
# buffer (-1 and 0 both land in the buffer or in the band in front of it), never a wild access.
POISON_A, POISON_B = "A", "B"
_INDEX_TYPES = (torch.int32, torch.int64, torch.uint8, torch.int8, torch.bool)


def poison_byte(poison: str, dtype: torch.dtype) -> int:
    if poison == POISON_A:
        return 0xFF
    if poison == POISON_B:
        return 0x00 if dtype in _INDEX_TYPES else 0x7B
    raise ValueError(f"poison {poison!r}: expected {POISON_A!r} or {POISON_B!r}")


_FACTORIES = ("empty", "empty_like", "zeros", "zeros_like", "full")
_METHODS = ("new_empty", "new_zeros", "new_full")


def _size_of(args, kw):
    """The size of a factory call: f(2, 3), f((2, 3)), f(torch.Size), f(size=...)."""
    if "size" in kw:
        args = (kw.pop("size"),)
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    return tuple(int(s) for s in args)


def _call_site():
    """(file, line) of the nearest frame outside this module: the factory call being served."""
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == __file__:
        f = f.f_back
    return (f.f_code.co_filename, f.f_lineno) if f is not None else None


class Allocation:
    """One guarded buffer: ``raw`` = the flat uint8 tensor (band | interior | band), ``lo`` .. ``hi`` = the interior's address range,
    ``site`` = (file, line) of the factory call that made it."""
    __slots__ = ("number", "raw", "nbytes", "shape", "dtype", "lo", "hi", "site")

    def __init__(self, number, raw, nbytes, shape, dtype, site=None):
        self.number, self.raw, self.nbytes, self.shape, self.dtype, self.site = number, raw, nbytes, shape, dtype, site
        self.lo = raw.data_ptr() + BAND
        self.hi = self.lo + nbytes

    def holds(self, addr: int) -> bool:
        return self.lo <= addr < self.hi or addr == self.lo


class Guard:
    """The state of one ``guarded`` context: ``allocations`` (in call order), ``empty`` / ``zeros`` / ``full`` for tests that pass
    ``out=`` or workspace tensors themselves, ``check_bands``."""

    def __init__(self, poison: str):
        poison_byte(poison, torch.float32)
        self.poison = poison
        self.allocations = []
        self._saved = {name: getattr(torch, name) for name in _FACTORIES}

    # ---- allocation (through the SAVED factories: the replaced ones would recurse)
    def _alloc(self, size, dtype, device, fill=None, requires_grad=False):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        n = math.prod(size)
        nbytes = n * dtype.itemsize
        raw = self._saved["empty"](nbytes + 2 * BAND, dtype=torch.uint8, device=device)
        raw.fill_(BAND_BYTE)
        inner = raw[BAND:BAND + nbytes]
        if fill is None:
            inner.fill_(poison_byte(self.poison, dtype))
        out = inner.view(dtype).view(size)
        if fill is not None:
            out.fill_(fill)
        self.allocations.append(Allocation(len(self.allocations), raw, nbytes, tuple(size), dtype, _call_site()))
        return out.requires_grad_() if requires_grad else out

    @staticmethod
    def _plain(kw) -> bool:
        """Only dense strided tensors are carved out of a byte buffer; anything else goes to the saved factory."""
        return kw.get("out") is None and kw.get("layout", torch.strided) is torch.strided and not kw.get("pin_memory", False)

    def _make(self, name, fill, args, kw):
        if not self._plain(kw):
            return self._saved[name](*args, **kw)
        kw = dict(kw)
        if name == "full":      # full(size, fill_value, ...)
            size, fill = (kw.pop("size") if "size" in kw else args[0]), (kw.pop("fill_value") if "fill_value" in kw else args[1])
            size = _size_of((size,), {})
            dtype = kw.get("dtype")
            if dtype is None:
                dtype = torch.tensor(fill).dtype if not isinstance(fill, float) else torch.get_default_dtype()
        else:
            size, dtype = _size_of(args, kw), kw.get("dtype")
        return self._alloc(size, dtype, kw.get("device"), fill, bool(kw.get("requires_grad", False)))

    def _make_like(self, name, fill, t, kw):
        fmt = kw.get("memory_format", torch.preserve_format)
        if not self._plain(kw) or fmt not in (torch.preserve_format, torch.contiguous_format) or not isinstance(t, torch.Tensor) or t.is_sparse:
            return self._saved[name](t, **kw)
        return self._alloc(tuple(t.shape), kw.get("dtype") or t.dtype, kw.get("device") or t.device, fill, bool(kw.get("requires_grad", False)))

    def empty(self, *args, **kw):
        return self._make("empty", None, args, kw)

    def zeros(self, *args, **kw):
        return self._make("zeros", 0, args, kw)

    def full(self, *args, **kw):
        return self._make("full", None, args, kw)

    def empty_like(self, t, **kw):
        return self._make_like("empty_like", None, t, kw)

    def zeros_like(self, t, **kw):
        return self._make_like("zeros_like", 0, t, kw)

    def _new(self, t, fill, args, kw):
        kw = dict(kw)
        kw.setdefault("dtype", t.dtype)
        kw.setdefault("device", t.device)
        return self._alloc(_size_of(args, kw), kw["dtype"], kw["device"], fill, bool(kw.get("requires_grad", False)))

    # ---- inspection
    def check_bands(self):
        """-> [(allocation number, shape, dtype, side, first, last)] of every band that no longer holds 0xA5.  ``side`` "before": the
        offsets count back from the interior's first byte (-1 = the byte in front of it); "after": from its end (0 = the first byte
        past it)."""
        bad = []
        for a in self.allocations:
            for side, band, origin in (("before", a.raw[:BAND], -BAND), ("after", a.raw[BAND + a.nbytes:], 0)):
                hit = (band != BAND_BYTE).nonzero()
                if hit.numel():
                    bad.append((a.number, a.shape, a.dtype, side, origin + int(hit[0]), origin + int(hit[-1])))
        return bad

    def find(self, addr: int):
        """The allocation whose interior holds ``addr``, or None."""
        return next((a for a in self.allocations if a.holds(addr)), None)


@contextlib.contextmanager
def guarded(poison: str):
    """Replace the tensor factories by guarded ones for the duration; restore them on exit, also when the body raises."""
    g = Guard(poison)
    patched = {"empty": g.empty, "zeros": g.zeros, "full": g.full, "empty_like": g.empty_like, "zeros_like": g.zeros_like}
    methods = {"new_empty": lambda t, *a, **k: g._new(t, None, a, k), "new_zeros": lambda t, *a, **k: g._new(t, 0, a, k),
               "new_full": lambda t, size, fill_value, **k: g._new(t, fill_value, (size,), k)}
    own = {m: torch.Tensor.__dict__.get(m) for m in _METHODS}     # (inherited from the C base class: nothing of their own to restore)
    try:
        for name, fn in patched.items():
            setattr(torch, name, fn)
        for name, fn in methods.items():
            setattr(torch.Tensor, name, fn)
        yield g
    finally:
        for name, fn in g._saved.items():
            setattr(torch, name, fn)
        for name, fn in own.items():
            if fn is None:
                delattr(torch.Tensor, name)
            else:
                setattr(torch.Tensor, name, fn)


# ------------------------------------------------------------------------------------------------ comparing bytes
def same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal dtype, shape and bytes (a NaN equals the same NaN)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.numel() == 0:
        return True
    return bool(torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))


def first_difference(a: torch.Tensor, b: torch.Tensor):
    """(flat element index of the first differing element, number of differing elements) of two tensors of one dtype and shape."""
    ab = a.contiguous().reshape(-1, 1).view(torch.uint8).reshape(a.numel(), -1)
    bb = b.contiguous().reshape(-1, 1).view(torch.uint8).reshape(b.numel(), -1)
    d = (ab != bb).any(-1).nonzero()
    return (int(d[0]), int(d.numel())) if d.numel() else (None, 0)


def byte_range(t: torch.Tensor):
    """The address range of a dense tensor, as ``unaccounted`` takes it for a declared input."""
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


# ------------------------------------------------------------------------------------------------ the recording proxy
def _address(a):
    """The address a pointer argument of a ctypes call carries (None / NULL -> 0)."""
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if isinstance(a, ctypes.c_void_p):
        return a.value or 0
    if hasattr(a, "_obj"):                       # ctypes.byref(x)
        return ctypes.addressof(a._obj)
    return ctypes.cast(a, ctypes.c_void_p).value or 0


def _struct_pointers(a):
    """[(label, address)] of the c_void_p fields of a descriptor array passed with ctypes.byref."""
    obj = getattr(a, "_obj", None)
    items = list(obj) if isinstance(obj, ctypes.Array) else ([obj] if isinstance(obj, ctypes.Structure) else [])
    out = []
    for i, s in enumerate(items):
        if isinstance(s, ctypes.Structure):
            out += [(f"[{i}].{name}", getattr(s, name) or 0) for name, tp in s._fields_ if tp is ctypes.c_void_p]
    return out


class RecordingLib:
    """Forwards every attribute to ``lib``; a call of an ``s2s_*`` export is recorded in ``calls`` as (name, [(position, address)]) for
    the positions ``signatures[name]`` types as c_void_p -- the pointer fields of a descriptor array as (f"{position}[i].field", address)
    -- before it is forwarded."""

    def __init__(self, lib, signatures):
        self._lib, self._signatures = lib, signatures
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("s2s_"):
            return fn
        sig = self._signatures.get(name, ())

        def call(*args):
            rec = []
            for i, a in enumerate(args):
                if i < len(sig) and sig[i] is ctypes.c_void_p:
                    rec.append((i, _address(a)))
                    rec += [(f"{i}{label}", addr) for label, addr in _struct_pointers(a)]
            self.calls.append((name, rec))
            return fn(*args)

        return call

    def exports(self):
        return {name for name, _ in self.calls}


def classify(addr: int, guard, declared, stream: int = 0) -> str:
    """"null" | "guarded" (inside an allocation of ``guard``) | "declared" (inside one of the (lo, hi) ranges) | "stream" | "foreign"."""
    if addr == 0:
        return "null"
    if guard is not None and guard.find(addr) is not None:
        return "guarded"
    if any(lo <= addr < hi or addr == lo for lo, hi in declared):
        return "declared"
    if addr == stream:
        return "stream"
    return "foreign"


def unaccounted(calls, guard, declared, stream: int = 0, host_arguments=()):
    """-> [(export, position)] of every recorded pointer that ``classify`` calls foreign and ``host_arguments`` (a collection of
    (export, position)) does not list.  The fields of a listed descriptor array are still checked one by one."""
    bad = []
    for name, rec in calls:
        for pos, addr in rec:
            if classify(addr, guard, declared, stream) == "foreign" and (name, pos) not in host_arguments:
                bad.append((name, pos))
    return bad
