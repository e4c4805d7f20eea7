"""Guard bands and poisoned buffers around every device entry point of include/str2str_kinetics.h: the discipline of tests/test_abi_bounds.py
carried over to the s2k_ family, built directly on tests/guarded_alloc.py (this module shares no state with test_abi_bounds.py, whose
completeness tests know the s2s_ exports only).

Every case runs twice on the ordinary allocator (the two must agree bit for bit) and once under each poison of ``guarded`` with the library
handle replaced by a recording proxy, and asserts for both guarded calls: every band intact; every pointer that reached the library NULL,
inside a guarded allocation, inside a declared tensor or the stream; every input equal to its clone as bytes (the documented in/out
argument -- the centres of s2k_centre_update -- is restored before each call and compared as a result); every returned tensor
byte-identical to the plain call's.  Nothing here has a tolerance.

Shapes: T in {1, 65, 257} (one frame; one past a wave; one past the 256-frame workgroup), d in {1, 3, 33} (the register paths below and
at a padded width, the LDS path), k in {1, 7, 65} (one past a wave of centres; with max_centres = 7 a tile ends inside the list).
GA.RecordingLib records the names that start with s2s_; ``Recorder`` below records the s2k_ ones the same way."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import guarded_alloc as GA
import kinetics_cases as KC

pytestmark = pytest.mark.gpu

DEV = "cuda"
RECORDED = set()        # every export a guarded call of this module reached
SITES = set()           # (file, line) of every factory call that was served by the guard


class Recorder(GA.RecordingLib):
    """GA.RecordingLib for the s2k_ exports: (name, [(position, address)]) of the positions the signature types as c_void_p."""

    def __getattr__(self, name):
        if not name.startswith("s2k_"):
            return super().__getattr__(name)
        fn, sig = getattr(self._lib, name), self._signatures.get(name, ())

        def call(*args):
            self.calls.append((name, [(i, GA._address(a)) for i, a in enumerate(args) if i < len(sig) and sig[i] is ctypes.c_void_p]))
            return fn(*args)

        return call


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def dev(a, dtype=None):
    return torch.as_tensor(np.array(a)).to(DEV, dtype).contiguous()


def run_case(name, call, inputs, inout=()):
    """``call(**inputs)`` -> a tuple of tensors.  ``inputs``: name -> tensor or None; ``inout``: the names the header documents as in/out."""
    from str2str_amd.ops import binding

    ins = {k: v for k, v in inputs.items() if v is not None}
    pristine = {k: v.clone() for k, v in ins.items()}
    declared = [GA.byte_range(v) for v in ins.values()]
    stream = torch.cuda.current_stream().cuda_stream
    signatures = {**binding._SIGNATURES, **binding._KINETICS_SIGNATURES}

    def once(poison):
        for k in inout:
            ins[k].copy_(pristine[k])
        report = []
        if poison is None:
            res = call(**inputs)
        else:
            proxy = Recorder(binding.load_library(), signatures)
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(binding, "_lib", proxy)
                with GA.guarded(poison) as g:
                    res = call(**inputs)
                    torch.cuda.synchronize()
                    bands = g.check_bands()
            RECORDED.update(proxy.exports())
            SITES.update(a.site for a in g.allocations)
            if not proxy.calls or not g.allocations:
                report.append(f"{name} [{poison}]: the call reached no entry point or allocated nothing through the guarded factories")
            if bands:
                report.append(f"{name} [{poison}]: bands written: {bands}")
            stray = GA.unaccounted(proxy.calls, g, declared, stream)
            if stray:
                report.append(f"{name} [{poison}]: pointers that are neither guarded nor declared: {sorted(set(map(str, stray)))}")
        torch.cuda.synchronize()
        for k, v in ins.items():
            if k not in inout and not GA.same_bytes(v, pristine[k]):
                report.append(f"{name} [{poison}]: input {k} was modified at element {GA.first_difference(v, pristine[k])[0]}")
        return [t.clone() for t in res if t is not None] + [ins[k].clone() for k in inout], report

    plain, report = once(None)
    plain2, _ = once(None)
    assert len(plain) == len(plain2)
    for i, (a, b) in enumerate(zip(plain, plain2)):
        assert GA.same_bytes(a, b), f"{name}: output {i} differs between two plain calls at element {GA.first_difference(a, b)}"
    for poison in (GA.POISON_A, GA.POISON_B):
        got, rep = once(poison)
        report += rep
        if len(got) != len(plain):
            report.append(f"{name} [{poison}]: {len(got)} outputs, {len(plain)} on the plain allocator")
        for i, (a, b) in enumerate(zip(got, plain)):
            if not GA.same_bytes(a, b):
                at = GA.first_difference(a, b) if a.shape == b.shape and a.dtype == b.dtype else (a.shape, b.shape)
                report.append(f"{name} [{poison}]: output {i} {tuple(b.shape)} {b.dtype} differs from the plain call: (first element, count) = {at}")
    assert not report, "\n".join(report)


def _inputs(T, d, k, seed=0):
    """Blob features, k centres out of a wider cloud (so that every centre is somebody's nearest or nobody's), labels with an unassigned one."""
    rng = np.random.default_rng([seed, T, d, k])
    x = KC.blobs(T, d, max(k, 2))
    centres = 6.0 * rng.standard_normal((k, d))
    labels = rng.integers(0, k, size=T).astype(np.int32)
    if T > 1:
        labels[T // 2] = -1
    return dev(x), dev(centres), dev(labels)


@pytest.mark.parametrize("T", KC.BOUNDS_T)
def test_assign(T):
    from str2str_amd import ops

    for d in KC.BOUNDS_D:
        for k in KC.BOUNDS_K:
            x, centres, prev = _inputs(T, d, k)
            run_case(f"assign T={T} d={d} k={k}", lambda **kw: ops.kmeans_assign(kw["x"], kw["centres"]), dict(x=x, centres=centres))
            run_case(f"assign T={T} d={d} k={k} prev, tiles of 7", lambda **kw: ops.kmeans_assign(kw["x"], kw["centres"], kw["prev"], max_centres=7),
                     dict(x=x, centres=centres, prev=prev))


@pytest.mark.parametrize("T", KC.BOUNDS_T)
def test_centre_update(T):
    from str2str_amd import ops

    for d in KC.BOUNDS_D:
        for k in KC.BOUNDS_K:
            x, centres, labels = _inputs(T, d, k)
            for segments in (None, 1):
                run_case(f"centre_update T={T} d={d} k={k} segments={segments}",
                         lambda **kw: (ops.kmeans_update(kw["x"], kw["labels"], kw["centres"], max_segments=segments),),
                         dict(x=x, labels=labels, centres=centres), inout=("centres",))


@pytest.mark.parametrize("T", KC.BOUNDS_T)
def test_farthest_point(T):
    from str2str_amd import ops

    for d in KC.BOUNDS_D:
        for k in sorted({min(k, T) for k in KC.BOUNDS_K}):          # the entry requires k <= T
            x = _inputs(T, d, k)[0]
            run_case(f"farthest_point T={T} d={d} k={k}", lambda **kw: ops.farthest_points(kw["x"], k, first=T // 2), dict(x=x))


@pytest.mark.parametrize("T", KC.BOUNDS_T)
def test_transition_counts(T):
    from str2str_amd import ops

    for k in KC.BOUNDS_K:
        labels = dev(KC.label_string(T, k))
        for lag in (1, 3):
            run_case(f"transition_counts T={T} k={k} lag={lag}", lambda **kw: (ops.transition_counts(kw["labels"], k, lag),), dict(labels=labels))
            lengths = dev(np.asarray(KC.split_lengths(T, 3)), torch.int32)
            run_case(f"transition_counts T={T} k={k} lag={lag}, 3 trajectories",
                     lambda **kw: (ops.transition_counts(kw["labels"], k, lag, kw["lengths"]),), dict(labels=labels, lengths=lengths))


# ------------------------------------------------------------------------------------------------ completeness (keep these tests last)
def test_every_kinetics_export_has_a_case():
    from str2str_amd.ops import binding

    want = set(binding.KINETICS_EXPORTS) - {"s2k_abi_version"}
    assert RECORDED == want, dict(no_case=sorted(want - RECORDED), unknown=sorted(RECORDED - want))


def test_every_allocation_site_of_the_wrappers_ran_guarded():
    """Every torch.empty / zeros / full call of ops/kinetics.py was served by the guard in some case of this module."""
    from str2str_amd.ops import kinetics

    path = os.path.abspath(kinetics.__file__)
    pat = re.compile(r"torch\.(empty|empty_like|zeros|zeros_like|full)\(|\.new_(empty|zeros|full)\(")
    with open(path) as f:
        sites = {(path, i + 1) for i, line in enumerate(f) if pat.search(line) and not line.lstrip().startswith("#")}
    reached = {(os.path.abspath(f), i) for f, i in SITES if f}
    print(f"allocation sites in ops/kinetics.py: {len(sites)}, reached: {len(sites & reached)}")
    assert len(sites) >= 10 and not sites - reached, sorted(i for _, i in sites - reached)
