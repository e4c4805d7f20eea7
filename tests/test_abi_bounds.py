"""Guard bands and poisoned buffers around every device entry point of include/str2str_hip.h.

A value comparison cannot see a kernel that stores past the end of its output (the caching allocator puts another tensor there, nothing
faults) or one whose result depends on what the allocator handed out (a ragged tail left unwritten, a workspace accumulated into but
never cleared, padding rows read into a softmax, a LayerNorm statistic or the range guard's maximum: the tests call the same shapes
again and again, so a fresh torch.empty very often holds the previous correct answer).  Here every case runs

    plain   twice on the ordinary allocator (they must agree bit for bit: the READMEs claim fixed summation orders),
    a, b    under tests/guarded_alloc.py's ``guarded`` with the poisons A (bytes 0xFF: NaN / -1) and B (bytes 0x7B: huge and finite;
            integers 0), the library handle replaced by the recording proxy,

and asserts, for both guarded calls: every band intact; every pointer that reached the library accounted for (inside a guarded
allocation, inside a declared tensor, NULL, the stream, or listed in HOST_ARGUMENTS / ALLOWED with its reason); every input equal to
its clone as bytes (but the documented in/out arguments, which are restored before each call and compared as results); the defined
region of every returned tensor byte-identical in a, b and plain; the range guard's eight words identical in a, b and plain, and zero.
The defined region is the whole tensor unless the case decodes it: ops.pair_untiled for a PairTiled (always), ops.unpack_planes for a
plane buffer, a column slice for an output at a column offset of a wider buffer, the first n rows of the native-contact list (the wrapper
returns exactly those).  Nothing here has a tolerance.

Shapes: the smallest at which a tail exists, not the workload's.

  family       unit                                         shapes
  pair stream  32-pair tiles                                B = 2, N in {1, 7, 33}: B N^2 = 2, 98, 2178, none a multiple of 32; with
                                                            S2S_ET_MAX_PAIRS / S2S_EE_MAX_PAIRS = N^2 + 7 a launch holds one sample and
                                                            ends inside a tile (row-major only: a tiled launch starts on a block)
  node stream  32-row tiles, 256-wide blocks                rows in {1, 33, 67}: below a tile, one row past a tile, three tiles with a tail
  attention    32-key tiles                                 B = 2, N in {7, 33, 65}, sample 0 with gaps in its mask, sample 1 a prefix
  geometry     256-thread blocks                            M in {1, 257}; se3_step and forward_marginal at N in {1, 65} (B = 3)
  ensemble     16 x 16 pair blocks, 48-blocks, 64-bit       R in {1, 17}, L in {1 where legal, 33, 65}, n_a x n_b = 17 x 5, chunks of 5
               words, 16 q, 64-lane spheres                 rows / structures (a chunk ends inside a block), Q = 17, P = 65 sphere points,
                                                            TICA (T, D, lag) = (97, 49, 2) and the grouped path at (1031, 10, 2)

One composed case runs a whole evaluation of the synthetic network under the guard (one kernel's padded output is the next one's input).
The last test holds the union of the exports the proxy saw against binding.EXPORTS: a new export without a case fails it.
"""
import copy
import os

import numpy as np
import pytest
import torch

import attention_cases as AC
import guarded_alloc as GA
import score_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (export, position): pointers that are host memory by the C ABI.
HOST_ARGUMENTS = {
    ("s2s_node_linear_multi", 0): "the s2s_node_problem descriptor array lives on the host (its pointer fields are checked one by one)",
    ("s2s_node_chain", 1): "the s2s_chain_layer descriptor array lives on the host (its pointer fields are checked one by one)",
}

# (export, position): read-only operands the wrapper stages itself with .to(device) / a comparison, so that no factory sees them.  The
# header declares every one of them const: the kernels cannot write them, and what they read is the caller's values.  No entry exempts a
# returned value, a band or an input of the test.
ALLOWED = {
    ("s2s_backbone_violations", 3): "atom_exists: `const unsigned char*` in the header; the wrapper normalises it to 0/1 ((t != 0).to(uint8))",
    ("s2s_backbone_sasa", 3): "atom_exists: `const unsigned char*` in the header; normalised to 0/1 by the wrapper",
    ("s2s_backbone_sasa", 4): "radii: `const double*` in the header; checked on the host as float64, then uploaded",
    ("s2s_backbone_sasa", 6): "sphere: `const double*` in the header; ops.sphere_points builds it on the host in numpy, then uploaded",
    ("s2s_ca_scattering", 3): "q: `const double*` in the header; a host array by the wrapper's contract, uploaded per call",
    ("s2s_ca_scattering", 5): "types: `const int*` in the header; a host array by the wrapper's contract, uploaded per call",
    ("s2s_ca_scattering", 6): "table: `const double*` in the header; a host array by the wrapper's contract, uploaded per call",
    ("s2s_ca_aligned_mean", 4): "p: `const double*` in the header; the sample weights are normalised on the host, then uploaded",
    ("s2s_ca_covariance", 4): "p: `const double*` in the header; the sample weights are normalised on the host, then uploaded",
}

HOST_ONLY = ("s2s_abi_version", "s2s_set_backbone_tables", "s2s_format_pdb_models", "s2s_write_pdb_models", "s2s_merge_pdb_files",
             "s2s_mt19937_discard")

# Cases whose two plain calls differ in bits (not run-to-run reproducible), with the reason and the bound of their parity test: none.
NOT_REPRODUCIBLE = {}

RECORDED = set()        # every export a guarded call of this module reached
STATS = {"guarded calls": 0, "guarded buffers": 0, "launches": 0}
SITES = set()           # (file, line) of every factory call that was served by the guard


# ------------------------------------------------------------------------------------------------ the harness
@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def net():
    from str2str_amd.factory import build_synthetic_net

    return build_synthetic_net(seed=0, sigma_final=0.02, device=DEV)


@pytest.fixture(scope="module")
def diffuser(tmp_path_factory):
    from str2str_amd.factory import build_diffuser

    return build_diffuser(str(tmp_path_factory.mktemp("so3cache")))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dev(t, dtype=None):
    t = torch.as_tensor(t)
    return t.to(DEV, dtype).contiguous()


def randn(g, *shape, dtype=torch.float32, scale=1.0):
    return dev(scale * torch.randn(*shape, generator=g, dtype=torch.float64), dtype)


def tensors_of(*objs):
    """Every tensor reachable from ``objs``: tensors, PairTiled, containers, modules and what their attributes hold (derived caches)."""
    from str2str_amd import ops

    seen, out, stack = set(), [], list(objs)
    while stack:
        o = stack.pop()
        if o is None or id(o) in seen or isinstance(o, (str, bytes, int, float, bool, type)):
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            out.append(o)
        elif isinstance(o, ops.PairTiled):
            out.append(o.buf)
        elif isinstance(o, dict):
            stack += list(dict.values(o))           # (a LazyDict's unbuilt entries stay unbuilt)
        elif isinstance(o, (list, tuple, set)):
            stack += list(o)
        elif isinstance(o, torch.nn.Module) or type(o).__module__.startswith("str2str_amd"):
            stack += list(vars(o).values()) if hasattr(o, "__dict__") else []
    return out


def flatten(result):
    """The tensors of a result in a fixed order; a PairTiled through its public decoder."""
    from str2str_amd import ops

    if result is None:
        return []
    if isinstance(result, torch.Tensor):
        return [result]
    if isinstance(result, ops.PairTiled):
        return [ops.pair_untiled(result)]
    if isinstance(result, dict):
        return [t for k in sorted(result) for t in flatten(result[k])]
    if isinstance(result, (list, tuple)):
        return [t for r in result for t in flatten(r)]
    raise TypeError(type(result))


def run_case(name, call, inputs, consts=(), inout=(), decode=None, flag_zero=True):
    """``call(alloc, **inputs)`` -> tensors; ``alloc`` is torch.empty on the plain runs and the guard's ``empty`` on the guarded ones (for
    cases that pass an ``out=`` themselves).  ``inputs``: name -> tensor / PairTiled / None, handed to every call as they are (the
    modules' derived caches key on the tensors' identity); ``inout``: the names the header documents as in/out -- restored before each
    call, compared as results after it.  ``consts``: what else the call reads (weights, tables, derived caches).  ``decode``: the
    defined region of the result, by default all of it."""
    from str2str_amd import ops
    from str2str_amd.ops import binding

    decode = decode or (lambda r: r)
    ins = {k: v for k, v in inputs.items() if v is not None}
    pristine = {k: [t.clone() for t in tensors_of(v)] for k, v in ins.items()}
    stream = torch.cuda.current_stream().cuda_stream

    def once(poison):
        for k in inout:
            for t, p in zip(tensors_of(ins[k]), pristine[k]):
                t.copy_(p)
        ops.range_flag_reset()
        report = []
        if poison is None:
            res = call(torch.empty, **inputs)
        else:
            proxy = GA.RecordingLib(binding.load_library(), binding._SIGNATURES)
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(binding, "_lib", proxy)
                with GA.guarded(poison) as g:
                    res = call(g.empty, **inputs)
                    torch.cuda.synchronize()
                    bands = g.check_bands()
            RECORDED.update(proxy.exports())
            STATS["guarded calls"] += 1
            STATS["guarded buffers"] += len(g.allocations)
            SITES.update(a.site for a in g.allocations)
            STATS["launches"] += len(proxy.calls)
            if not proxy.calls or not (g.allocations or inout):
                report.append(f"{name} [{poison}]: the call reached no entry point or allocated nothing through the guarded factories")
            if bands:
                report.append(f"{name} [{poison}]: bands written: {bands}")
            stray = GA.unaccounted(proxy.calls, g, declared, stream, set(HOST_ARGUMENTS) | set(ALLOWED))
            if stray:
                report.append(f"{name} [{poison}]: pointers that are neither guarded nor declared: {sorted(set(map(str, stray)))}")
        torch.cuda.synchronize()
        for k, v in ins.items():
            if k not in inout:
                for i, (t, p) in enumerate(zip(tensors_of(v), pristine[k])):
                    if not GA.same_bytes(t, p):
                        report.append(f"{name} [{poison}]: input {k}[{i}] was modified at element {GA.first_difference(t, p)[0]}")
        out = [t.clone() for t in flatten(decode(res))] + [t.clone() for k in inout for t in flatten(ins[k])]
        return out, ops.range_flag().tolist(), report

    call(torch.empty, **inputs)                       # warm-up: derived caches, tables, the range flag's buffer
    for k in inout:
        for t, p in zip(tensors_of(ins[k]), pristine[k]):
            t.copy_(p)
    declared = [GA.byte_range(t) for t in tensors_of(ins, list(consts), ops.range_flag())]
    plain, flag, report = once(None)
    plain2, flag2, _ = once(None)
    assert len(plain) == len(plain2) and name not in NOT_REPRODUCIBLE
    for i, (x, y) in enumerate(zip(plain, plain2)):
        assert GA.same_bytes(x, y), f"{name}: output {i} differs between two plain calls at element {GA.first_difference(x, y)}"
    assert flag == flag2
    for poison in (GA.POISON_A, GA.POISON_B):
        got, gflag, rep = once(poison)
        report += rep
        if len(got) != len(plain):
            report.append(f"{name} [{poison}]: {len(got)} outputs, {len(plain)} on the plain allocator")
        for i, (x, y) in enumerate(zip(got, plain)):
            if not GA.same_bytes(x, y):
                at = GA.first_difference(x, y) if x.shape == y.shape and x.dtype == y.dtype else (x.shape, y.shape)
                report.append(f"{name} [{poison}]: output {i} {tuple(y.shape)} {y.dtype} differs from the plain call: (first element, count) = {at}")
        if gflag != flag:
            report.append(f"{name} [{poison}]: range words {gflag}, plain {flag}")
    if flag_zero and any(flag):
        report.append(f"{name}: range words {flag} for in-range inputs ({ops.range_flag_names(flag[0])})")
    assert not report, "\n".join(report)


def planes(n_rows, k, *cols):
    """Decoder of a plane buffer [n_rows, k]: ops.unpack_planes, columns ``cols`` = (c0, c1) if only those are written."""
    from str2str_amd import ops

    c0, c1 = cols if cols else (0, k)
    return lambda xp: ops.unpack_planes(xp, n_rows, k)[:, c0:c1].contiguous()


def packed_inside(call, *names):
    """``call`` with its fp32 inputs ``names`` packed into planes INSIDE the call: under the guard the padding rows of the planes (a buffer
    holds whole 32-row tiles) are then poison -- in production they are whatever the block held -- and not the zeros or the earlier
    answer a buffer made ahead of the case would carry."""
    def f(alloc, **kw):
        from str2str_amd import ops

        for n in names:
            kw[n] = ops.pack_planes(kw[n])
        return call(alloc, **kw)
    return f


# ------------------------------------------------------------------------------------------------ node stream
ROWS = (1, 33, 67)


def _layer(g, n_out, k, whole=False):
    from str2str_amd import ops

    w = randn(g, n_out, k, scale=k ** -0.5)
    return ops.pack_node_layer(w, randn(g, n_out, scale=0.1), whole)


@pytest.mark.parametrize("M", ROWS)
def test_pack_planes(M):
    from str2str_amd import ops

    g = gen(100 + M)
    x, rs = randn(g, M, 320), randn(g, M).abs() + 0.5
    run_case(f"pack_planes M={M}", lambda alloc, x, rs: ops.pack_planes(x), dict(x=x, rs=rs), decode=planes(M, 320))

    def offset(alloc, x, rs):      # columns 64 .. 320 of x, scaled per row, into k-steps 4 .. of a 320-wide buffer
        out = alloc(ops.xp_alloc(M, 320, DEV).numel(), dtype=torch.int16, device=DEV)
        return ops.pack_planes(x, 64, 256, out, 320, 64, rs)

    run_case(f"pack_planes M={M} at a column offset", offset, dict(x=x, rs=rs), decode=planes(M, 320, 64, 320))


@pytest.mark.parametrize("M", ROWS)
def test_node_linear(M):
    from str2str_amd import ops

    g = gen(200 + M)
    x = randn(g, M, 256)
    res, pm, qm = randn(g, M, 256), dev((torch.rand(M, generator=g) > 0.3).float()), dev((torch.rand(M, generator=g) > 0.3).float())
    gamma, beta = randn(g, 256).abs() + 0.5, randn(g, 256)
    wide, whole = _layer(g, 512, 256), _layer(g, 256, 256, True)
    consts = [wide, whole, wide["w"], whole["w"], wide["w32"], whole["w32"]]

    def plain16(alloc, xp, **_):
        return ops.node_linear(xp, wide["w"], wide["b"], M, 256, 512, wide["tg"], relu=True, want_f32=True, want_xp=True)

    run_case(f"node_linear M={M}", packed_inside(plain16, "xp"), dict(xp=x), consts, decode=lambda r: (r[0], planes(M, 512)(r[1])))

    def ln16(alloc, xp, res, pm, qm, gamma, beta):    # every epilogue option; both outputs at a column offset of 320-wide buffers
        o32 = alloc(M, 320, dtype=torch.float32, device=DEV)
        oxp = alloc(ops.xp_alloc(M, 320, DEV).numel(), dtype=torch.int16, device=DEV)
        return ops.node_linear(xp, whole["w"], whole["b"], M, 256, 256, whole["tg"], pre_mask=pm, residual=res, ln=(gamma, beta, 1e-5), post_mask=qm,
                               out_f32=o32, out_col0=64, out_xp=oxp, out_xp_k=320, out_xp_k0=64)

    run_case(f"node_linear M={M} LayerNorm epilogue at a column offset", packed_inside(ln16, "xp"), dict(xp=x, res=res, pm=pm, qm=qm, gamma=gamma, beta=beta), consts,
             decode=lambda r: (r[0][:, 64:].contiguous(), planes(M, 320, 64, 320)(r[1])))

    def f32(alloc, x, res, pm, qm, gamma, beta):
        o = alloc(M, 320, dtype=torch.float32, device=DEV)
        a = ops.node_linear_f32(x, wide["w32"], wide["b"], M, 256, 512, wide["tg"], relu=True)
        b = ops.node_linear_f32(x, whole["w32"], whole["b"], M, 256, 256, whole["tg"], pre_mask=pm, residual=res, ln=(gamma, beta, 1e-5),
                                post_mask=qm, out=o, out_col0=64)
        return a, b[:, 64:].contiguous()

    run_case(f"node_linear_f32 M={M}", f32, dict(x=x, res=res, pm=pm, qm=qm, gamma=gamma, beta=beta), consts)

    # the row map of the attention operands: output row (sample, n) of n_pad rows from input row sample * n_src + min(n, n_src - 1)
    n_src = max(1, M // 2)
    n_pad = ops.padded_len(n_src)
    xs = randn(g, 2 * n_src, 256)
    run_case(f"node_linear M={M} row map",
             packed_inside(lambda alloc, xs: ops.node_linear(xs, wide["w"], wide["b"], 2 * n_pad, 256, 512, wide["tg"], want_f32=False, want_xp=True,
                                                             row_map=(n_pad, n_src))[1], "xs"),
             dict(xs=xs), consts, decode=planes(2 * n_pad, 512))


@pytest.mark.parametrize("M", ROWS)
def test_node_linear_vfrag_multi_chain_layernorm(M, net):
    from str2str_amd import ops

    g = gen(300 + M)
    xp = randn(g, M, 256)      # (fp32: every case packs it inside its call, ``packed_inside``)
    ipa = net.translator.trunk["ipa_0"]
    w = ipa.node_packs()
    consts = [ipa]
    run_case(f"node_linear_vfrag M={M}", packed_inside(lambda alloc, xp: ops.node_linear_vfrag(xp, w["v"]["w"], w["v"]["b"], M, 256, 2048, 8), "xp"),
             dict(xp=xp), consts)

    a, b, c = _layer(g, 256, 256), _layer(g, 256, 256), _layer(g, 256, 256, True)
    two = [a, b]
    consts2 = [a, b, c, [L[k] for L in (a, b, c) for k in ("w", "w_s", "w_row")]]
    scale = randn(g, M).abs() + 0.5

    def multi(alloc, xp, scale):
        o = alloc(M, 512, dtype=torch.float32, device=DEV)
        return ops.node_apply_multi(xp, [(two[0], dict(out_f32=o, out_col0=0, relu=True)), (two[1], dict(out_f32=o, out_col0=256, pre_scale=scale)),
                                         (c, dict(want_f32=False, want_xp=True))], M)

    run_case(f"node_linear_multi M={M}", packed_inside(multi, "xp"), dict(xp=xp, scale=scale), consts2,
             decode=lambda r: (r[0][0], planes(M, 256)(r[2][1])))

    NP = ops.padded_len(M)
    run_case(f"node_linear_multi M={M} (ipa_projections, row map)",
             packed_inside(lambda alloc, xp: ops.ipa_projections(xp, w["q"], w["k"], w["v"], w["qp"], w["kvp"], M, NP, (NP, M) if NP != M else None), "xp"),
             dict(xp=xp), consts, decode=lambda r: (planes(NP, 2048)(r[0]), planes(NP, 2048)(r[1]), r[2], r[3], r[4]))

    res, gamma, beta, qm = randn(g, M, 256), randn(g, 256).abs() + 0.5, randn(g, 256), dev((torch.rand(M, generator=g) > 0.3).float())
    mid = randn(g, M, 256)

    def chain(alloc, xp, res, gamma, beta, qm, mid):
        m_out = alloc(M, 256, dtype=torch.float32, device=DEV)
        o32, oxp = ops.node_chain(xp, [a["w_row"], b["w_row"], c["w_row"]], [a["b"], b["b"], c["b"]], [False, True, False], M, 256, residual=res,
                                  ln_gamma=gamma, ln_beta=beta, ln_eps=1e-5, post_mask=qm, want_f32=True, want_xp=True, mid_residual=mid,
                                  mid_out_f32=m_out, mid_ln=(gamma, beta, 1e-5))
        return o32, oxp, m_out

    run_case(f"node_chain M={M}", packed_inside(chain, "xp"), dict(xp=xp, res=res, gamma=gamma, beta=beta, qm=qm, mid=mid), consts2,
             decode=lambda r: (r[0], planes(M, 256)(r[1]), r[2]))

    xw = randn(g, M, 320)
    run_case(f"row_layernorm M={M}",
             lambda alloc, xw, gamma, beta, qm: ops.row_layernorm(xw, M, 256, gamma, beta, 1e-5, qm, want_f32=True, want_xp=True),
             dict(xw=xw, gamma=gamma, beta=beta, qm=qm), decode=lambda r: (r[0], planes(M, 256)(r[1])))


# ------------------------------------------------------------------------------------------------ pair stream
PAIR_N = (1, 7, 33)


def pair_inputs(N, seed):
    from str2str_amd import ops

    B, g = 2, gen(seed)
    edge = randn(g, B, N, N, 128)
    ab = randn(g, B, N, 896)
    ab[..., 384:] *= 32.0                                      # the kernel form: column half and G at the accumulators' scale
    ab[..., 768:] -= ab[..., 768:].mean(-1, keepdim=True)      # ... and G centred
    n_p = randn(g, B, N, 128)
    mask = torch.ones(B, N)
    mask[1, N // 2:] = 0.0                                     # a different mask per sample (N = 1: sample 1 all off)
    return dict(edge=edge, tiled=ops.pair_tiled(edge), ab=ab.contiguous(), n_p=n_p, mask=dev(mask))


@pytest.mark.parametrize("N", PAIR_N)
def test_edge_transition_f16x3(N, net, monkeypatch):
    from str2str_amd import ops

    et, nxt = net.translator.trunk["edge_transition_0"], net.translator.trunk["ipa_1"].pair_proj_weights()
    pk = et._packed()
    stream = torch.cat([pk["wstream_f16"], nxt["wp_f16x2"]])
    ln = et.layer_norm
    consts = [et, net.translator.trunk["ipa_1"], stream, nxt["wp_f16x2"]]
    ins = pair_inputs(N, 400 + N)

    def call(src, lay, with_proj):
        def f(alloc, edge, tiled, ab, n_p, mask):
            return ops.edge_transition_f16x3(tiled if src == "tiled" else edge, ab, n_p, stream if with_proj else pk["wstream_f16"], et.trunk[2].bias,
                                             ln.weight, ln.bias, mask, ln.eps, proj=(stream, nxt["b64"]) if with_proj else None, out_layout=lay,
                                             ab_kernel_form=True)
        return f

    for src, lay, with_proj in (("rowmajor", "rowmajor", False), ("rowmajor", "rowmajor", True), ("rowmajor", "tiled", False), ("tiled", "tiled", True),
                                ("tiled", "rowmajor", False), ("tiled", "none", True)):
        run_case(f"edge_transition_f16x3 N={N} {src} -> {lay} proj={with_proj}", call(src, lay, with_proj), ins, consts)

    def chained(alloc, edge, tiled, ab, n_p, mask):
        """A tiled tensor a kernel wrote -- its padding pairs are whatever the buffer held: poison here -- read by the next launch."""
        t1 = call("rowmajor", "tiled", False)(alloc, edge, tiled, ab, n_p, mask)
        return t1, call("tiled", "tiled", True)(alloc, edge, t1, ab, n_p, mask)

    run_case(f"edge_transition_f16x3 N={N} tiled output into the next launch", chained, ins, consts)
    # the trunk's form (torch.ops.str2str_amd.edge_transition_f16x3_chain), through its only caller
    run_case(f"edge_transition_f16x3_chain N={N}",
             lambda alloc, edge, tiled, ab, n_p, mask: et.pair_mlp(tiled, ab, n_p, mask, nxt, out_layout="tiled", ab_kernel_form=True), ins, consts)
    if N > 1:      # a launch per sample: N^2 = 49 | 1089 pairs, so the second launch starts inside a 32-pair tile
        monkeypatch.setenv("S2S_ET_MAX_PAIRS", str(N * N + 7))
        run_case(f"edge_transition_f16x3 N={N} split launches", call("rowmajor", "rowmajor", True), ins, consts)


@pytest.mark.parametrize("N", PAIR_N)
def test_edge_transition_f32_and_pair_project(N, net):
    from str2str_amd import ops

    et, ipa = net.translator.trunk["edge_transition_0"], net.translator.trunk["ipa_1"]
    nxt, pk, ln = ipa.pair_proj_weights(), et._packed_f32(), et.layer_norm
    consts = [et, ipa]
    ins = pair_inputs(N, 500 + N)
    ins["ab"] = ins["ab"][..., :768].contiguous()
    del ins["tiled"]
    for with_proj in (False, True):
        run_case(f"edge_transition N={N} proj={with_proj}",
                 lambda alloc, edge, ab, n_p, mask: ops.edge_transition(edge, ab, n_p, pk["w1p"], pk["w2p"], pk["wfp"], et.trunk[2].bias, et._bf_centred(),
                                                                        ln.weight, ln.bias, mask, ln.eps,
                                                                        proj=(nxt["wp"], nxt["b64"]) if with_proj else None), ins, consts)
    run_case(f"pair_project N={N}", lambda alloc, edge: ops.pair_project(edge, nxt["wp"], nxt["b64"]), dict(edge=ins["edge"]), consts)


def embed_inputs(emb, N, seed):
    B, g = 2, gen(seed)
    idx = torch.arange(N)[None].repeat(B, 1)
    idx[:, N // 2:] += 3                                       # a gap in the numbering
    fixed = (torch.rand(B, N, generator=g) > 0.6).float()
    if N > 1:
        fixed[0, 0], fixed[0, 1] = 0.0, 1.0                    # both values occur: four (fa, fb) classes
    mask = torch.ones(B, N)
    mask[1, N // 2:] = 0.0
    ca = 8.0 * torch.randn(B, N, 3, generator=g)
    from str2str_amd.models.net.denoising_ipa import get_timestep_embedding

    t_img = emb.time_images(get_timestep_embedding(torch.tensor([0.37]), 32))[0].contiguous()
    return dict(residue_idx=idx, fixed_mask=dev(fixed), ca=dev(ca), node_mask=dev(mask), t_img=t_img)


@pytest.mark.parametrize("N", PAIR_N)
@pytest.mark.parametrize("config", ["f16x3", "f16x3-classes", "f32"])
def test_embedder(N, config, net, monkeypatch):
    """embed_assemble, the node MLP (node_chain | node_linear_f32) and the edge embedding of the configuration -- through
    EmbeddingModule.embed, the only caller of embed_assemble -- row-major and tiled, with and without the fused projection."""
    emb = copy.deepcopy(net.embedder)
    ipa = net.translator.trunk["ipa_0"]
    nxt = ipa.pair_proj_weights()
    nxt["wp_f16x2"]
    emb.arith = "f32" if config == "f32" else "f16x3"
    emb.ee_classes = "1" if config.endswith("classes") else "0"
    ins = embed_inputs(emb, N, 600 + N)

    def call(layout, with_proj):
        def f(alloc, residue_idx, fixed_mask, ca, node_mask, t_img):
            node, act, edge, proj = emb.embed(residue_idx, None, fixed_mask, ca, node_mask, nxt if with_proj else None, edge_layout=layout, t_img=t_img)
            return node, edge, proj
        return f

    consts = [emb, ipa]
    layouts = ("rowmajor",) if config == "f32" else ("rowmajor", "tiled")
    for layout in layouts:
        for with_proj in (False, True):
            call(layout, with_proj)(torch.empty, **ins)       # (the caches of this combination, before they are declared)
            run_case(f"embedder {config} N={N} {layout} proj={with_proj}", call(layout, with_proj), ins, consts)
    if N > 1 and config != "f32":
        monkeypatch.setenv("S2S_EE_MAX_PAIRS", str(N * N + 7))
        run_case(f"embedder {config} N={N} split launches", call("rowmajor", True), ins, consts)


# ------------------------------------------------------------------------------------------------ attention
ATT_N = (7, 33, 65)


def attention_inputs(N, seed):
    B, g = 2, gen(seed)
    mask = torch.stack([AC.mask_of("gaps", N, g), AC.mask_of("prefix-half", N, g)])
    s = torch.randn(B, N, 256, generator=g) * mask[..., None]
    r7 = torch.cat([AC.random_rotations(B * N, g).view(B, N, 4), AC.chain_walk(B, N, g)], -1).float()
    return dict(s=dev(s), bias=dev(torch.randn(B, 8, N, N, generator=g)), pz=dev(torch.randn(B, N, N, 32, generator=g)), r7=dev(r7), mask=dev(mask))


@pytest.mark.parametrize("N", ATT_N)
def test_ipa_attention_f32(N, net):
    from str2str_amd import ops

    B, M = 2, 2 * N
    ipa = net.translator.trunk["ipa_0"]
    w, d = ipa.node_packs(), ipa._derived()
    c = attention_inputs(N, 700 + N)
    s_xp = ops.pack_planes(c["s"].reshape(M, -1))
    q, kv, qp, kvp = (ops.node_apply(s_xp, w[k], M)[0] for k in ("q", "kv", "qp", "kvp"))
    consts = [ipa]
    r7, mask = c["r7"], c["mask"]
    run_case(f"ipa_prep_points N={N}", lambda alloc, r7, qp, kvp: ops.ipa_prep_points(r7, qp.view(B, N, -1), kvp.view(B, N, -1)),
             dict(r7=r7, qp=qp, kvp=kvp), consts)
    pts = ops.ipa_prep_points(r7, qp.view(B, N, -1), kvp.view(B, N, -1))
    ins = dict(q=q.view(B, N, 8, -1), kv=kv.view(B, N, 8, -1), q_pts=pts[0], k_pts=pts[1], v_pts=pts[2], bias=c["bias"], pz=c["pz"], mask=mask, r7=r7)
    for inplace in (False, True):
        run_case(f"ipa_attention + ipa_opair N={N} logits_inplace={inplace}",
                 lambda alloc, q, kv, q_pts, k_pts, v_pts, bias, pz, mask, r7: ops.ipa_attention(q, kv, q_pts, k_pts, v_pts, bias, pz, mask, r7, d["hw"],
                                                                                                logits_inplace=inplace),
                 ins, consts, inout=("bias",) if inplace else ())


@pytest.mark.parametrize("N", ATT_N + (32,))      # (32: whole tiles -- the bias array itself can take the logits, s itself is the shared K operand)
@pytest.mark.parametrize("fold", [True, False], ids=["shared-kv", "per-head"])
def test_ipa_attention_f16(N, fold, net):
    from str2str_amd import ops

    B, M = 2, 2 * N
    ipa = copy.deepcopy(net.translator.trunk["ipa_0"])
    ipa.arith, ipa.fold = "f16x3", fold
    w, d = ipa.node_packs(), ipa._derived()
    c = attention_inputs(N, 800 + N)
    s2d = c["s"].reshape(M, -1).contiguous()
    s_xp = ops.pack_planes(s2d)
    qp, kvp = (ops.node_apply(s_xp, w[k], M)[0] for k in ("qp", "kvp"))
    r7, mask = c["r7"], c["mask"]
    ipa.attention(s_xp, B, N, r7, mask, (c["bias"].clone(), c["pz"]))
    consts = [ipa]
    # the points of a block: every array is defined on its padded rows too (zero points, k2 = -1e9): compared whole
    run_case(f"ipa_prep_points_f16 N={N} fold={fold}",
             packed_inside(lambda alloc, r7, qp, kvp, s_xp: ops.ipa_prep_points_f16(r7, qp, kvp, d["hw"], s_xp=s_xp if fold else None), "s_xp"),
             dict(r7=r7, qp=qp, kvp=kvp, s_xp=s2d), consts)
    # projections -> points -> core -> pair term -> the o_pt / o_pair columns packed behind the o columns: through the block's method,
    # which hands the core the bias for its logits (logits_inplace where the length is a multiple of 32)
    run_case(f"ipa_attention_f16w + ipa_opair N={N} fold={fold}",
             packed_inside(lambda alloc, s_xp, r7, mask, bias, pz: ipa.attention(s_xp, B, N, r7, mask, (bias, pz)), "s_xp"),
             dict(s_xp=s2d, r7=r7, mask=mask, bias=c["bias"], pz=c["pz"]), consts, inout=("bias",), decode=planes(M, 2688))
    if not fold:
        NP = ops.padded_len(N)

        def direct(alloc, s_xp, r7, mask, bias, pz):
            """The wrapper itself, the logits in a buffer of their own: (fp32 features, their o_pt / o_pair columns valid; planes, their o
            columns valid) -- the defined regions as ops.ipa_attention_f16 documents them."""
            q_xp, k_xp, v_vf, qp, kvp = ops.ipa_projections(s_xp, w["q"], w["k"], w["v"], w["qp"], w["kvp"], M, B * NP, (NP, N) if NP != N else None)
            feats, fxp = ops.ipa_attention_f16(q_xp, k_xp, v_vf, ops.ipa_prep_points_f16(r7, qp, kvp, d["hw"]), bias, pz, mask, r7)
            return feats[..., 2048:].contiguous(), planes(M, 2688, 0, 2048)(fxp)

        run_case(f"ipa_attention_f16 N={N}, logits not in place", packed_inside(direct, "s_xp"),
                 dict(s_xp=s2d, r7=r7, mask=mask, bias=c["bias"], pz=c["pz"]), consts)


@pytest.mark.parametrize("N", ATT_N)
@pytest.mark.parametrize("arith", ["f32", "f16x3"])
def test_encoder_attention(N, arith):
    from str2str_amd import ops

    B, g = 2, gen(900 + N)
    qkv = randn(g, B * N, 960)
    kb = torch.zeros(B, N)
    kb[0] = 1.0 - AC.mask_of("gaps", N, g)                     # the reference's float padding, added to the logits
    kb[1, (N + 1) // 2:] = float("-inf")                       # exact padding: a prefix of keys
    for name, key_bias in (("no key bias", None), ("key bias", dev(kb))):
        run_case(f"encoder_attention {arith} N={N} {name}",
                 lambda alloc, qkv, key_bias: ops.encoder_attention(qkv, key_bias, B, N, 4, want_f32=True, want_xp=True, arith=arith),
                 dict(qkv=qkv, key_bias=key_bias), decode=lambda r: (r[0], planes(B * N, 320)(r[1])))


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("M", [1, 257])
def test_frame_kernels(M):
    from str2str_amd import ops

    g = gen(1000 + M)
    r7 = dev(torch.cat([AC.random_rotations(M, g), 10.0 * torch.randn(M, 3, generator=g, dtype=torch.float64)], -1).float())
    upd6, upd32 = randn(g, M, 6, scale=0.1), randn(g, M, 32, scale=0.1)
    mask = dev((torch.rand(M, generator=g) > 0.2).float())
    run_case(f"rigid_compose_update M={M}", lambda alloc, r7, upd6, mask: ops.rigid_compose_update(r7, upd6, mask), dict(r7=r7, upd6=upd6, mask=mask))
    run_case(f"rigid_compose_update M={M} padded update", lambda alloc, r7, upd32, mask: ops.rigid_compose_update(r7, upd32, mask),
             dict(r7=r7, upd32=upd32, mask=mask))
    for divide in (False, True):
        run_case(f"rigid_scale_trans M={M} divide={divide}", lambda alloc, r7: ops.rigid_scale_trans(r7, 0.1, divide), dict(r7=r7))
    u, gt, fixed = randn(g, M, 32), randn(g, M, 7, 2), dev((torch.rand(M, generator=g) > 0.5).float())
    run_case(f"torsion_head M={M}", lambda alloc, u: ops.torsion_head(u, M), dict(u=u))
    run_case(f"torsion_head M={M} blended", lambda alloc, u, gt, fixed: ops.torsion_head(u, M, True, 1e-8, gt[..., 2, :], fixed), dict(u=u, gt=gt, fixed=fixed))
    psi = torch.nn.functional.normalize(randn(g, M, 2), dim=-1).contiguous()
    aatype = dev(torch.randint(0, 20, (M,), generator=g))
    for a37, a14 in ((True, False), (False, True), (True, True)):
        run_case(f"frames_to_backbone M={M} atom37={a37} atom14={a14}",
                 lambda alloc, r7, psi, aatype: ops.frames_to_backbone(r7, psi, aatype, want_atom37=a37, want_atom14=a14), dict(r7=r7, psi=psi, aatype=aatype))
    run_case(f"frames_to_backbone M={M} no aatype", lambda alloc, r7, psi: ops.frames_to_backbone(r7, psi, None), dict(r7=r7, psi=psi))


@pytest.mark.parametrize("N", [1, 65])
def test_se3_step(N, diffuser):
    from str2str_amd import ops

    c = SC.score_case(N, diffuser)
    B, g = SC.SCORE_B, gen(1100 + N)
    ins = dict(x0=dev(c["x0"]), xt=dev(c["xt"]), mask=dev(c["mask"]), dm=dev(c["mask"] * (torch.rand(B, N, generator=g) > 0.2).float()), p8=dev(c["p8"]),
               z_rot=randn(g, B, N, 3, dtype=torch.float64), z_trans=randn(g, B, N, 3, dtype=torch.float64),
               dt=dev(torch.tensor([0.01, 0.02, 0.005], dtype=torch.float64)))
    fused = lambda alloc, x0, xt, mask, dm, p8, z_rot, z_trans, dt: ops.se3_step(x0, xt, mask, dm, p8, 0.01, probability_flow=False,  # noqa: E731
                                                                                 z_rot=z_rot, z_trans=z_trans, want_next=True, want_scores=True)
    run_case(f"se3_step N={N} fused, with scores", fused, ins)
    run_case(f"se3_step N={N} fused, without scores, probability flow, per-sample dt",
             lambda alloc, x0, xt, mask, dm, p8, z_rot, z_trans, dt: ops.se3_step(x0, xt, mask, dm, p8, dt), ins)
    run_case(f"se3_step N={N} split: scores only",
             lambda alloc, x0, xt, mask, dm, p8, z_rot, z_trans, dt: ops.se3_step(x0, xt, mask, dm, p8, 0.0, want_next=False, want_scores=True), ins)
    _, rs, ts = ops.se3_step(ins["x0"], ins["xt"], ins["mask"], ins["dm"], ins["p8"], 0.0, want_next=False, want_scores=True)
    ins2 = dict(ins, rs=rs, ts=ts)
    del ins2["x0"]
    run_case(f"se3_step N={N} split: the step from given scores",
             lambda alloc, xt, mask, dm, p8, z_rot, z_trans, dt, rs, ts: ops.se3_step(None, xt, mask, dm, p8, 0.01, probability_flow=False, z_rot=z_rot,
                                                                                      z_trans=z_trans, rot_score_in=rs, trans_score_in=ts), ins2)


@pytest.mark.parametrize("N", [1, 65])
def test_forward_marginal(N, diffuser):
    from str2str_amd import ops

    c = SC.fm_case(N, diffuser)
    ins = dict(rig0=dev(c["rig0"]), z_axis=dev(c["z_axis"]), u=dev(c["u"]), z_trans=dev(c["z_trans"]), cdf=dev(c["cdf"]),
               rows=dev(torch.tensor(c["rows"], dtype=torch.int32)), omega=dev(c["omega"]), p2=dev(c["params2"]), dm=dev(c["diffuse_mask"]))
    run_case(f"forward_marginal N={N} noising",
             lambda alloc, rig0, z_axis, u, z_trans, cdf, rows, omega, p2, dm: ops.forward_marginal(rig0, z_axis, u, z_trans, cdf, rows, omega, p2, dm), ins)
    run_case(f"forward_marginal N={N} prior",
             lambda alloc, rig0, z_axis, u, z_trans, cdf, rows, omega, p2, dm: ops.forward_marginal(None, z_axis, u, z_trans, cdf, rows, omega, None), ins)


# ------------------------------------------------------------------------------------------------ ensemble metrics
def chains(R, L, seed, spread=1.0):
    """R noisy copies of one random 3.8 A chain walk [R, L, 3] float32 on the device."""
    g = gen(seed)
    step = torch.randn(L, 3, generator=g, dtype=torch.float64)
    base = (3.8 * step / step.norm(dim=-1, keepdim=True)).cumsum(0)
    x = base[None] + spread * torch.randn(R, L, 3, generator=g, dtype=torch.float64)
    return dev(x - x.mean(1, keepdim=True), torch.float32)


def backbone(R, L, seed):
    """[R, L, 5, 3]: N, CA, C, O, CB about a chain walk (geometry does not matter here: every kernel must write its outputs anyway)."""
    g = gen(seed)
    ca = chains(R, L, seed).cpu().double()
    off = torch.tensor([[-1.2, 0.6, 0.0], [0.0, 0.0, 0.0], [1.3, 0.7, 0.0], [1.5, 1.9, 0.2], [0.2, -1.0, 1.1]], dtype=torch.float64)
    return dev(ca[:, :, None, :] + off + 0.2 * torch.randn(R, L, 5, 3, generator=g, dtype=torch.float64), torch.float32)


ENS = [(R, L) for R in (1, 17) for L in (1, 33, 65)]


@pytest.mark.parametrize("R,L", ENS)
def test_ca_statistics_and_distances(R, L):
    from str2str_amd import ops

    ca, ref = chains(R, L, 2000 + 10 * R + L), chains(5, L, 2100 + L)
    if L > 1:      # (the entry point refuses a single residue: there is no adjacent pair)
        run_case(f"ca_sample_stats R={R} L={L}", lambda alloc, ca: ops.ca_sample_stats(ca, 3.0, 1), dict(ca=ca))
    if L > 3:
        w_ref, w = dev(torch.rand(5, generator=gen(1), dtype=torch.float64) + 0.1), dev(torch.rand(R, generator=gen(2), dtype=torch.float64) + 0.1)
        run_case(f"ca_pairwise_distances R={R} L={L}", lambda alloc, ca: ops.ca_pairwise_distances(ca, 1), dict(ca=ca))
        run_case(f"ca_pwd_js R={R} L={L}", lambda alloc, ref, ca: ops.ca_pwd_js(ref, ca), dict(ref=ref, ca=ca))
        run_case(f"ca_pwd_js R={R} L={L} weighted", lambda alloc, ref, ca, w_ref, w: ops.ca_pwd_js(ref, ca, ref_weights=w_ref, pred_weights=w),
                 dict(ref=ref, ca=ca, w_ref=w_ref, w=w))


@pytest.mark.parametrize("L", [1, 33, 65])
def test_pair_matrices(L):
    """n_a x n_b = 17 x 5 in row chunks of 5: a chunk ends inside a 16 x 16 pair block."""
    from str2str_amd import ops

    a, b = chains(17, L, 2200 + L), chains(5, L, 2300 + L)
    w = dev(torch.rand(L, generator=gen(3)) + 0.1)
    ins = dict(a=a, b=b)
    run_case(f"ca_rmsd_matrix L={L}", lambda alloc, a, b: ops.ca_rmsd_matrix(a, b, max_pairs=25), ins)
    run_case(f"ca_rmsd_matrix L={L} weighted, self", lambda alloc, a, w: ops.ca_rmsd_matrix(a, None, w), dict(a=a, w=w))
    run_case(f"ca_tm_matrix L={L}", lambda alloc, a, b: ops.ca_tm_matrix(a, b, max_pairs=25), ins)
    run_case(f"ca_tm_matrix L={L} self", lambda alloc, a: ops.ca_tm_matrix(a), dict(a=a))
    run_case(f"ca_lddt_matrix L={L}", lambda alloc, a, b: ops.ca_lddt_matrix(a, b, max_pairs=25), ins)
    run_case(f"ca_lddt_matrix L={L} self", lambda alloc, a: ops.ca_lddt_matrix(a), dict(a=a))


@pytest.mark.parametrize("R,L", ENS)
def test_superpositions(R, L):
    from str2str_amd import ops

    ca, target = chains(R, L, 2400 + 10 * R + L), chains(1, L, 2500 + L)[0].contiguous()
    w = dev(torch.rand(L, generator=gen(4)) + 0.1)
    run_case(f"ca_superpose R={R} L={L}", lambda alloc, ca, target: ops.ca_superpose(ca, target), dict(ca=ca, target=target))
    run_case(f"ca_superpose R={R} L={L} weighted", lambda alloc, ca, target, w: ops.ca_superpose(ca, target, w), dict(ca=ca, target=target, w=w))
    run_case(f"ca_tm_superpose R={R} L={L}", lambda alloc, ca, target: ops.ca_tm_superpose(ca, target), dict(ca=ca, target=target))
    run_case(f"ca_lddt_per_residue R={R} L={L}", lambda alloc, ca, target: ops.ca_lddt_per_residue(ca, target), dict(ca=ca, target=target))
    xform = ops.ca_superpose(ca, target)[1]
    pts = backbone(R, L, 2600 + L).reshape(R, L * 5, 3).contiguous()
    run_case(f"apply_xform R={R} L={L}", lambda alloc, pts, xform: ops.apply_xform(pts, xform), dict(pts=pts, xform=xform))


@pytest.mark.parametrize("R,L", ENS)
def test_backbone_kernels(R, L):
    """Violations, secondary structure, SASA (P = 65 sphere points) and scattering (Q = 17, three bead types), in launches of 5 structures."""
    from str2str_amd import ops

    g = gen(2700 + 10 * R + L)
    atoms = backbone(R, L, 2800 + 10 * R + L)
    aatype, idx = dev(torch.randint(0, 20, (L,), generator=g), torch.int32), torch.arange(L)
    idx[L // 2:] += 2
    idx = dev(idx, torch.int32)
    exists = torch.ones(L, 5, dtype=torch.uint8)
    exists[::3, 4] = 0
    exists = dev(exists)
    radii = torch.tensor([1.65, 1.87, 1.76, 1.4, 1.87], dtype=torch.float64).repeat(L, 1)
    run_case(f"backbone_violations R={R} L={L}", lambda alloc, atoms, exists, aatype, idx: ops.backbone_violations(atoms, exists, aatype, idx, max_structures=5),
             dict(atoms=atoms, exists=exists, aatype=aatype, idx=idx))
    run_case(f"secondary_structure R={R} L={L}", lambda alloc, atoms, aatype, idx: ops.secondary_structure(atoms, aatype, idx, max_structures=5),
             dict(atoms=atoms, aatype=aatype, idx=idx))
    run_case(f"backbone_sasa R={R} L={L}", lambda alloc, atoms, exists: ops.backbone_sasa(atoms, exists, radii, n_points=65, max_structures=5),
             dict(atoms=atoms, exists=exists))
    ca = atoms[:, :, 1].contiguous()
    q = np.linspace(0.0, 0.6, 17)
    types = np.arange(L) % 3
    table = 1.0 + 0.1 * np.arange(3)[:, None] - 0.5 * q[None, :]
    run_case(f"ca_scattering R={R} L={L}", lambda alloc, ca: ops.ca_scattering(ca, q, types, table, max_structures=5), dict(ca=ca))
    run_case(f"ca_scattering R={R} L={L} one type", lambda alloc, ca: ops.ca_scattering(ca, q[:1]), dict(ca=ca))


@pytest.mark.parametrize("R,L", ENS)
def test_contacts(R, L):
    from str2str_amd import ops

    ca, native = chains(R, L, 2900 + 10 * R + L, 0.5), chains(1, L, 2900 + 10 * R + L, 0.0)[0].contiguous()
    w = dev(torch.rand(R, generator=gen(5), dtype=torch.float64) + 0.1)
    run_case(f"ca_contact_map R={R} L={L}", lambda alloc, ca: ops.ca_contact_map(ca)[0], dict(ca=ca))
    run_case(f"ca_contact_map R={R} L={L} weighted", lambda alloc, ca, w: ops.ca_contact_map(ca, weights=w), dict(ca=ca, w=w))
    run_case(f"ca_contact_stats R={R} L={L}", lambda alloc, ca: ops.ca_contact_stats(ca), dict(ca=ca))
    # (the wrapper returns the first n rows of its list buffers, n the count it read back: the defined region)
    run_case(f"ca_native_contacts L={L}", lambda alloc, native: ops.ca_native_contacts(native, 10.0, 3), dict(native=native))
    pairs, d0 = ops.ca_native_contacts(native, 10.0, 3)
    assert pairs.shape[0] > 0 or L < 4
    run_case(f"ca_native_q R={R} L={L}", lambda alloc, ca, pairs, d0: ops.ca_native_q(ca, pairs, d0), dict(ca=ca, pairs=pairs, d0=d0))


@pytest.mark.parametrize("R,L", ENS)
def test_essential_dynamics(R, L):
    """sym48_f64.h through the PCA kernels: 3 L = 3, 99, 195 coordinates (one ragged 48-block, three, five), chunks of 8 structures of 17."""
    from str2str_amd import ops

    ca = chains(R, L, 3000 + 10 * R + L)
    xform = ops.ca_superpose(ca, ca[0].contiguous())[1]
    p = torch.rand(R, generator=gen(6), dtype=torch.float64) + 0.1
    run_case(f"ca_aligned_mean R={R} L={L}", lambda alloc, ca, xform: ops.ca_aligned_mean(ca, xform), dict(ca=ca, xform=xform))
    run_case(f"ca_aligned_mean R={R} L={L} weighted, no transform", lambda alloc, ca: ops.ca_aligned_mean(ca, None, p), dict(ca=ca))
    mean = ops.ca_aligned_mean(ca, xform)
    run_case(f"ca_covariance R={R} L={L}", lambda alloc, ca, mean, xform: ops.ca_covariance(ca, mean, xform, max_structures=5), dict(ca=ca, mean=mean, xform=xform))
    run_case(f"ca_covariance R={R} L={L} weighted", lambda alloc, ca, mean, xform: ops.ca_covariance(ca, mean, xform, p), dict(ca=ca, mean=mean, xform=xform))
    comps = randn(gen(7), 3, 3 * L, dtype=torch.float64)
    run_case(f"ca_project R={R} L={L}", lambda alloc, ca, mean, comps, xform: ops.ca_project(ca, mean, comps, xform), dict(ca=ca, mean=mean, comps=comps, xform=xform))


@pytest.mark.parametrize("T,D,lag,max_pairs", [(97, 49, 2, 20), (97, 49, 2, None), (1031, 10, 2, 64), (5, 1, 1, None)])
def test_time_lagged_covariances(T, D, lag, max_pairs):
    """sym48_f64.h through the TICA kernels: D = 49 (a 48-block and one column), the grouped path (more than one group) at D = 10, the
    workspace in steps that end inside a group."""
    from str2str_amd import ops

    f = randn(gen(3100 + T), T, D)
    assert (ops.tica_groups(T - lag, D)[0] > 1) == (T > 1000)
    run_case(f"lagged_mean {T, D, lag}", lambda alloc, f: ops.lagged_mean(f, lag), dict(f=f))
    mean = ops.lagged_mean(f, lag)
    run_case(f"lagged_covariances {T, D, lag} max_pairs={max_pairs}", lambda alloc, f, mean: ops.lagged_covariances(f, mean, lag, max_pairs), dict(f=f, mean=mean))
    comps = randn(gen(8), 3, D, dtype=torch.float64)
    run_case(f"feature_project {T, D}", lambda alloc, f, mean, comps: ops.feature_project(f, mean, comps), dict(f=f, mean=mean, comps=comps))


@pytest.mark.parametrize("n", [1, 17, 65, 130])
def test_clustering(n):
    """64-bit words: n = 17 (a partial word), 65 (one bit in the second), 130; the adjacency in two row chunks, the second into the
    buffers of the first (in/out by the header)."""
    from str2str_amd import ops

    ca = chains(n, 9, 3200 + n, 2.0)
    values = ops.ca_rmsd_matrix(ca)
    cutoff = float(values.median())
    run_case(f"cluster_adjacency n={n}", lambda alloc, values: ops.cluster_adjacency(values, cutoff), dict(values=values))
    if n > 1:
        k = n // 2 + 1
        first, rest = values[:k].contiguous(), values[k:].contiguous()
        run_case(f"cluster_adjacency n={n} first row chunk", lambda alloc, first: ops.cluster_adjacency(first, cutoff), dict(first=first))
        adj, deg = ops.cluster_adjacency(first, cutoff)
        run_case(f"cluster_adjacency n={n} second row chunk", lambda alloc, rest, adj, deg: ops.cluster_adjacency(rest, cutoff, row0=k, adj=adj, deg=deg),
                 dict(rest=rest, adj=adj, deg=deg), inout=("adj", "deg"))
    adj, deg = ops.cluster_adjacency(values, cutoff)
    run_case(f"cluster_gromos n={n}", lambda alloc, adj, deg: ops.cluster_gromos(adj, deg, rounds_per_sync=3), dict(adj=adj, deg=deg))


# ------------------------------------------------------------------------------------------------ one evaluation of the network
def test_one_network_evaluation(net, monkeypatch):
    """build_synthetic_net(seed=0, sigma_final=0.02), B = 2, N = 37, three residues off in the last sample, arithmetic f16x3, no HIP graph:
    embedder -> trunk, every buffer between the kernels guarded and poisoned.  The frames, psi and the embedder's pair tensor are
    byte-identical in a, b and plain, the bands intact, the range flag zero.  (The modules stage some operands with torch operators that
    no factory sees -- views, casts, concatenations: the pointers of this case are recorded for the completeness test, not classified.)"""
    from str2str_amd import ops
    from str2str_amd.ops import binding
    from str2str_amd.models.net.denoising_ipa import get_timestep_embedding

    monkeypatch.setenv("S2S_HIP_GRAPH", "0")
    B, N, g = 2, 37, gen(4000)
    m = copy.deepcopy(net)
    for mod in m.modules():
        if hasattr(mod, "arith"):
            assert mod.arith == "f16x3"
    mask = torch.ones(B, N)
    mask[1, [3, 20, 36]] = 0.0
    r7 = torch.cat([AC.random_rotations(B * N, g).view(B, N, 4), 10.0 * AC.chain_walk(B, N, g)], -1).float()
    batch = dict(residue_idx=torch.arange(N)[None].repeat(B, 1), t=torch.full((B,), 0.37), fixed_mask=dev(torch.zeros(B, N)), residue_mask=dev(mask),
                 sc_ca_t=dev(r7[..., 4:]), rigids_t=dev(r7), torsion_angles_sin_cos=dev(torch.nn.functional.normalize(torch.randn(B, N, 7, 2, generator=g), dim=-1)),
                 t_img=m.embedder.time_images(get_timestep_embedding(torch.tensor([0.37]), 32))[0].contiguous())

    def evaluate():
        nxt = m.translator.trunk["ipa_0"].pair_proj_weights()
        node, act, edge, proj = m.embedder.embed(batch["residue_idx"], batch["t"], batch["fixed_mask"], batch["sc_ca_t"], batch["residue_mask"], nxt,
                                                 edge_layout="tiled", t_img=batch["t_img"])
        out = m.translator(node, edge, dict(batch, _node_embed_act=act), _first_proj=proj)
        torch.cuda.synchronize()
        return [out["out_rigids7"].clone(), out["psi"].clone(), ops.pair_untiled(edge), node.clone()]

    evaluate()
    ops.range_flag_reset()
    plain = evaluate()
    assert all(GA.same_bytes(x, y) for x, y in zip(plain, evaluate())), "the evaluation is not run-to-run reproducible"
    assert ops.range_flag().tolist() == [0] * 8
    keep = {k: v.clone() for k, v in batch.items()}
    for poison in (GA.POISON_A, GA.POISON_B):
        proxy = GA.RecordingLib(binding.load_library(), binding._SIGNATURES)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(binding, "_lib", proxy)
            with GA.guarded(poison) as guard:
                got = evaluate()
                bands = guard.check_bands()
        RECORDED.update(proxy.exports())
        SITES.update(a.site for a in guard.allocations)
        print(f"network evaluation [{poison}]: {len(guard.allocations)} guarded buffers, {len(proxy.calls)} launches")
        assert not bands, bands
        for name, x, y in zip(("rigids", "psi", "edge", "node"), got, plain):
            assert GA.same_bytes(x, y), (poison, name, GA.first_difference(x, y))
        assert all(GA.same_bytes(batch[k], keep[k]) for k in batch), "an input was modified"
        assert ops.range_flag().tolist() == [0] * 8, ops.range_flag().tolist()


# ------------------------------------------------------------------------------------------------ completeness (keep these tests last)
def test_every_device_export_has_a_case():
    from str2str_amd.ops import binding

    want = set(binding.EXPORTS) - set(HOST_ONLY)
    print(STATS)
    seen = RECORDED - set(HOST_ONLY)
    assert seen == want, dict(no_case=sorted(want - seen), unknown=sorted(seen - want))
    assert all(isinstance(v, str) and v for v in list(HOST_ARGUMENTS.values()) + list(ALLOWED.values()))


# The modules of str2str_amd/ops whose factory calls make what a kernel writes or reads (range_guard.py's one buffer lives for the whole
# process: every case declares it), and the calls among them that make no kernel operand: (file, a fragment of the line) -> why.
KERNEL_WRAPPERS = ("attention", "ensemble", "geometry", "node", "pair", "packing")
NO_KERNEL_OPERAND = {
    ("packing.py", "w.new_zeros(pad"): "_pad_rows32: a weight packer in plain torch, run once per weight (the tests build packed weights ahead of the guard)",
    ("packing.py", "b = w.new_zeros(n_pad"): "pack_node_layer: the padded bias of a packed layer, built with the weights ahead of the guard",
    ("packing.py", "zp = torch.zeros("): "pair_tiled: the test-side converter into the tiled layout, plain torch",
    ("packing.py", "out = torch.zeros(fr.shape[0]"): "unpack_planes: the test-side decoder of plane buffers, plain torch",
    ("packing.py", "else torch.empty(n_rows, k, device=device"): "act_alloc: its fp32 branch has no caller in the package",
}


def test_every_allocation_site_of_the_wrappers_ran_guarded():
    """Every torch.empty / zeros / full (and _like, new_*) call in the kernel wrappers was served by the guard in some case of this module:
    a new output or workspace that no case reaches fails here."""
    import re

    from str2str_amd.ops import binding

    root = os.path.dirname(os.path.abspath(binding.__file__))
    pat = re.compile(r"torch\.(empty|empty_like|zeros|zeros_like|full)\(|\.new_(empty|zeros|full)\(")
    sites = set()
    for mod in KERNEL_WRAPPERS:
        path = os.path.join(root, mod + ".py")
        with open(path) as f:
            sites |= {(path, i + 1) for i, line in enumerate(f) if pat.search(line) and not line.lstrip().startswith("#")
                      and not any(name == mod + ".py" and frag in line for name, frag in NO_KERNEL_OPERAND)}
    reached = {(os.path.abspath(f), i) for f, i in SITES if f}
    print(f"allocation sites in the wrappers: {len(sites)}, reached: {len(sites & reached)}")
    assert len(sites) > 80 and not sites - reached, sorted((os.path.basename(f), i) for f, i in sites - reached)
