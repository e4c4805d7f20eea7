"""tests/guarded_alloc.py on the CPU, against planted mistakes: eight small torch functions standing in for a kernel and its wrapper,
each wrong in one of the ways the device test (tests/test_abi_bounds.py) exists to catch, and each caught by the assertion meant for
it -- the bands, the comparison of the two poisons with a plain call, or the comparison of the inputs with their clones.  A correct
function passes all of them.  Then the helper's own contract: the views it returns, the restoring of the factories, the proxy.

A "kernel" here writes through a flat view that starts at its buffer's address and runs past its end (``torch.as_strided`` on the
underlying storage), as a device kernel would through a raw pointer.
"""
import ctypes

import pytest
import torch

import guarded_alloc as GA

ROWS, COLS = 5, 8


def stray_store(t, first, value):
    """Store ``value`` into the element ``first`` elements from ``t``'s first one, wherever that is in its storage: what a kernel holding
    ``t``'s pointer can reach.  On the plain allocator the element is outside the tensor's own storage -- a device kernel would corrupt
    a neighbour there; the stand-in has none and skips the store."""
    at = t.storage_offset() + first
    if 0 <= at and (at + 1) * t.element_size() <= t.untyped_storage().nbytes():
        torch.as_strided(t, (1,), (1,), at).fill_(value)


# ---------------------------------------------------------------------------------------------------- the stand-ins
def correct(x):
    out = torch.empty(ROWS, COLS)
    out.copy_(2.0 * x)
    return out


def one_past_the_end(x):
    out = correct(x)
    stray_store(out, out.numel(), 3.0)
    return out


def one_before_the_start(x):
    out = correct(x)
    stray_store(out, -1, 3.0)
    return out


def stray_row_far_behind(x):
    """A whole row whose first byte lies BAND - 1 bytes past the end: one byte of it is still inside the band."""
    out = torch.empty(ROWS, COLS, dtype=torch.uint8)
    out.copy_(x[:, :COLS].to(torch.uint8))
    stray_store(out, out.numel() + GA.BAND - 1, 7)      # (the rest of the row would leave the memory the guard owns)
    return out


def last_row_unwritten(x):
    out = torch.empty(ROWS, COLS)
    out[:-1] = 2.0 * x[:-1]
    return out


def accumulates_into_empty(x):
    ws = torch.empty(COLS)
    for r in range(ROWS):
        ws += x[r]
    return ws.clone()


def max_over_padded_row(x):
    """Rows padded to 16 columns; the maximum runs over the padding too."""
    buf = torch.empty(ROWS, 16)
    buf[:, :COLS] = x
    return buf.amax(-1)


def modifies_its_input(x):
    out = correct(x)
    x[0, 0] += 1.0
    return out


def int_output_unwritten(x):
    idx = torch.empty(ROWS, dtype=torch.int32)
    idx[:-1] = torch.arange(ROWS - 1, dtype=torch.int32)
    return idx


def judge(fn, x):
    """The assertions of the device test, by name -> the set of those that fail for ``fn``."""
    failed = set()
    plain = fn(x.clone())
    runs = {}
    for poison in (GA.POISON_A, GA.POISON_B):
        xin = x.clone()
        keep = xin.clone()
        with GA.guarded(poison) as g:
            runs[poison] = fn(xin)
            if g.check_bands():
                failed.add("bands")
        if not GA.same_bytes(xin, keep):
            failed.add("inputs")
    a, b = runs[GA.POISON_A], runs[GA.POISON_B]
    if not (GA.same_bytes(a, b) and GA.same_bytes(a, plain)):
        failed.add("outputs")
    return failed


@pytest.fixture
def x():
    return torch.randn(ROWS, COLS, generator=torch.Generator().manual_seed(7)).abs() + 0.5


def test_a_correct_function_passes(x):
    assert judge(correct, x) == set()


@pytest.mark.parametrize("fn, caught_by", [
    (one_past_the_end, "bands"), (one_before_the_start, "bands"), (stray_row_far_behind, "bands"), (last_row_unwritten, "outputs"),
    (accumulates_into_empty, "outputs"), (max_over_padded_row, "outputs"), (modifies_its_input, "inputs"), (int_output_unwritten, "outputs")],
    ids=lambda v: v.__name__ if callable(v) else v)
def test_planted_mistake_is_caught(x, fn, caught_by):
    assert judge(fn, x) == {caught_by}


def test_band_reports_say_where(x):
    with GA.guarded(GA.POISON_A) as g:
        one_past_the_end(x)
        assert g.check_bands() == [(0, (ROWS, COLS), torch.float32, "after", 0, 3)]
    with GA.guarded(GA.POISON_A) as g:
        one_before_the_start(x)
        assert g.check_bands() == [(0, (ROWS, COLS), torch.float32, "before", -4, -1)]
    with GA.guarded(GA.POISON_B) as g:
        stray_row_far_behind(x)
        assert g.check_bands() == [(0, (ROWS, COLS), torch.uint8, "after", GA.BAND - 1, GA.BAND - 1)]


# ---------------------------------------------------------------------------------------------------- the views
def test_band_is_a_multiple_of_512_bytes_and_four_pair_tiles():
    assert GA.BAND % 512 == 0 and GA.BAND == 4 * 32 * 128 * 4


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64, torch.int16, torch.int32, torch.int64, torch.uint8])
@pytest.mark.parametrize("shape", [(3, 5), (7,), (0,), (4, 0, 2), (2, 3, 4, 5)])
def test_views_are_contiguous_aligned_and_typed(dtype, shape):
    with GA.guarded(GA.POISON_A) as g:
        made = [torch.empty(*shape, dtype=dtype), torch.empty(shape, dtype=dtype), torch.zeros(shape, dtype=dtype),
                torch.full(shape, 3, dtype=dtype), torch.empty_like(torch.ones(shape, dtype=dtype).t() if len(shape) == 2 else torch.ones(shape, dtype=dtype)),
                torch.zeros_like(torch.ones(shape, dtype=dtype)), torch.ones(2).new_empty(shape, dtype=dtype), torch.ones(2, dtype=dtype).new_zeros(shape),
                torch.ones(2, dtype=dtype).new_full(shape, 3), g.empty(shape, dtype=dtype)]
        assert len(g.allocations) == len(made)
        for t, a in zip(made, g.allocations):
            want = tuple(reversed(shape)) if (t is made[4] and len(shape) == 2) else shape
            assert t.dtype == dtype and tuple(t.shape) == want and t.is_contiguous()
            assert t.data_ptr() == (a.lo if t.numel() else 0)        # (torch reports NULL for a tensor without elements)
            assert (a.lo - a.raw.data_ptr()) % 512 == 0 and a.hi - a.lo == t.numel() * t.element_size()
            assert a.raw.numel() == a.nbytes + 2 * GA.BAND
        assert g.check_bands() == []
    n = 1
    for s in shape:
        n *= s
    if n:
        assert bool((made[2] == 0).all()) and bool((made[3] == 3).all()) and bool((made[5] == 0).all()) and bool((made[7] == 0).all()) and bool((made[8] == 3).all())


def test_poisons():
    with GA.guarded(GA.POISON_A):
        f16, f32, f64, i32, i64, u8 = (torch.empty(4, dtype=d) for d in (torch.float16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8))
    assert all(bool(torch.isnan(t).all()) for t in (f16, f32, f64))
    assert bool((i32 == -1).all()) and bool((i64 == -1).all()) and bool((u8 == 255).all())
    with GA.guarded(GA.POISON_B):
        f16, f32, f64, i16, i32, i64, u8 = (torch.empty(4, dtype=d) for d in (torch.float16, torch.float32, torch.float64, torch.int16, torch.int32,
                                                                              torch.int64, torch.uint8))
    assert float(f16[0]) == 61280.0 and float(f16[0]) >= 2.0 ** 15 and 1.2e36 < float(f32[0]) < 1.4e36 and 1e285 < float(f64[0]) < 1e287
    assert float(i16.view(torch.float16)[0]) == 61280.0                     # the f16 planes travel as int16
    assert bool((i32 == 0).all()) and bool((i64 == 0).all()) and bool((u8 == 0).all())


def test_factories_are_restored_after_an_exception():
    before = [getattr(torch, n) for n in GA._FACTORIES] + [getattr(torch.Tensor, n) for n in GA._METHODS]
    with pytest.raises(RuntimeError, match="planted"):
        with GA.guarded(GA.POISON_A):
            assert torch.empty is not before[0]
            raise RuntimeError("planted")
    assert [getattr(torch, n) for n in GA._FACTORIES] + [getattr(torch.Tensor, n) for n in GA._METHODS] == before
    assert not any(n in torch.Tensor.__dict__ for n in GA._METHODS)
    assert not bool(torch.isnan(torch.zeros(3)).any())


def test_the_helper_does_not_recurse_and_counts_only_the_callers_allocations():
    with GA.guarded(GA.POISON_A) as g:
        torch.empty(3)
        g.check_bands()
        torch.zeros(2, 2)
    assert [a.shape for a in g.allocations] == [(3,), (2, 2)]
    assert all(a.site[0] == __file__ for a in g.allocations) and g.allocations[1].site[1] == g.allocations[0].site[1] + 2    # where it was asked for


# ---------------------------------------------------------------------------------------------------- the proxy
class _Desc(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("n", ctypes.c_int), ("out", ctypes.c_void_p)]


class _FakeLib:
    def __init__(self):
        self.seen = []
        self.other = "not an export"

    def s2s_fake(self, *args):
        self.seen.append(args)
        return 0

    def s2s_fake_multi(self, *args):
        return 0


def test_proxy_classifies_pointers():
    vp, i = ctypes.c_void_p, ctypes.c_int
    fake = _FakeLib()
    lib = GA.RecordingLib(fake, {"s2s_fake": [vp, vp, i, vp, vp, vp], "s2s_fake_multi": [vp, i, vp]})
    assert lib.other == "not an export"
    declared_t, foreign_t = torch.ones(16), torch.ones(16)
    stream = 0x5000
    with GA.guarded(GA.POISON_A) as g:
        out = torch.empty(8)
        rc = lib.s2s_fake(vp(declared_t.data_ptr() + 8), vp(out.data_ptr()), 3, None, vp(foreign_t.data_ptr()), vp(stream))
        arr = (_Desc * 2)()
        arr[0].w, arr[0].out = declared_t.data_ptr(), out.data_ptr()
        arr[1].w, arr[1].out = foreign_t.data_ptr(), 0
        lib.s2s_fake_multi(ctypes.byref(arr), 2, None)
    assert rc == 0 and len(fake.seen) == 1 and fake.seen[0][2] == 3                      # forwarded, untouched
    (name, rec), (name2, rec2) = lib.calls
    assert name == "s2s_fake" and [p for p, _ in rec] == [0, 1, 3, 4, 5]                # the int at position 2 is no pointer
    declared = [GA.byte_range(declared_t)]
    assert [GA.classify(a, g, declared, stream) for _, a in rec] == ["declared", "guarded", "null", "foreign", "stream"]
    assert GA.classify(out.data_ptr() + out.numel() * 4, g, declared, stream) == "foreign"     # one past a guarded interior: in the band
    assert GA.unaccounted(lib.calls[:1], g, declared, stream) == [("s2s_fake", 4)]
    assert GA.unaccounted(lib.calls[:1], g, declared, stream, {("s2s_fake", 4)}) == []
    # a descriptor array: the array itself is a host argument, its pointer fields are checked one by one
    assert [p for p, _ in rec2] == [0, "0[0].w", "0[0].out", "0[1].w", "0[1].out", 2]
    assert GA.unaccounted(lib.calls[1:], g, declared, stream, {("s2s_fake_multi", 0)}) == [("s2s_fake_multi", "0[1].w")]
    assert lib.exports() == {"s2s_fake", "s2s_fake_multi"}
