"""Node stream: the per-node dense layers, their fused forms, and the policy that picks a kernel form for a layer (``node_apply*``)."""
import ctypes
from typing import Optional

import torch

from .binding import HipLibraryError, _check, _int_arg, _p, _req, _req_all, _req_opt, _stream, _timed, load_library
from .packing import vf_alloc, xp_alloc
from .range_guard import range_flag

SMALL_ROWS = 8192        # at or below: a long contraction with a row-normalising epilogue runs as narrow GEMM + LayerNorm (node_apply)
NARROW_MAX_WORK = 24 << 20   # rows x output columns up to which the narrow column blocks ("tg_s") of a layer are the faster form
#   (tools/node_gemm_bench.py --tg 2 against the default, profiles/r04_node_gemm_small_m.txt: 2048 columns win up to ~10 k rows and
#    lose from ~24 k, 512 .. 960 columns still win at 24 k rows)
CHAIN_WIDTHS = (256, 320)    # output widths s2s_node_chain is instantiated for


def _ln_args(ln, name=None):
    """``ln`` = (gamma, beta, eps) or None -> the three LayerNorm arguments of a launch; with ``name`` the tensors are checked under it."""
    if ln is None:
        return None, None, 0.0
    g, b, eps = ln
    if name:
        _req(g, name=name + ".gamma"); _req(b, name=name + ".beta")
    return g, b, float(eps)


def _node_outputs(n_rows: int, n_out: int, dev, out_f32, want_f32, out_xp, out_xp_k, want_xp):
    """The output convention of the node layers -> (out_f32, out_xp, out_xp_k): each buffer is the caller's or, when wanted, allocated
    here ([n_rows, n_out] fp32 first, then packed planes); ``out_xp_k``, the width of the planes buffer, defaults to ``n_out``."""
    if out_f32 is None and want_f32:
        out_f32 = torch.empty(n_rows, n_out, device=dev, dtype=torch.float32)
    if out_xp_k is None and (out_xp is not None or want_xp):
        out_xp_k = n_out
    if out_xp is None and want_xp:
        out_xp = xp_alloc(n_rows, out_xp_k, dev)
    return out_f32, out_xp, out_xp_k


def pack_planes(x2d: torch.Tensor, col0: int = 0, n_cols: Optional[int] = None, out=None, out_k: Optional[int] = None, k0: int = 0, row_scale=None):
    """fp32 [M, ld] (columns col0 .. col0 + n_cols) -> XP planes, optionally into columns k0.. of a wider XP buffer."""
    lib = load_library()
    _req(x2d, name="x")
    M, ld = x2d.shape
    n_cols = ld - col0 if n_cols is None else n_cols
    out_k = n_cols if out_k is None else out_k
    out = xp_alloc(M, out_k, x2d.device) if out is None else out
    _req_opt(row_scale=row_scale)
    _check(lib.s2s_pack_planes(_p(x2d), M, ld, col0, n_cols, _p(out), out_k // 16, k0 // 16, _p(row_scale), _p(range_flag()), _stream()), "s2s_pack_planes")
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
    map_pad, map_src = row_map if row_map is not None else (0, 0)
    in_rows = n_rows // map_pad * map_src if map_pad else n_rows
    _req_opt(bias=bias, pre_scale=pre_scale, pre_mask=pre_mask, residual=residual, post_mask=post_mask)
    if xp.numel() != ((in_rows + 31) // 32) * (k_in // 16) * 1024 or wpk.numel() != n_out * k_in * 2:
        raise HipLibraryError(f"node_linear: operand sizes do not match M={in_rows} K={k_in} N={n_out}")
    out_f32, out_xp, out_xp_k = _node_outputs(n_rows, n_out, xp.device, out_f32, want_f32, out_xp, out_xp_k, want_xp)
    _req_opt(out_f32=out_f32)
    _req_opt(torch.int16, out_xp=out_xp)
    g, b, eps = _ln_args(ln, "ln")
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_linear(
        _p(xp), _p(wpk), _p(bias), n_rows, k_in, n_out, tiles, _p(pre_scale), int(bool(relu)), _p(pre_mask), _p(residual),
        residual.shape[-1] if residual is not None else 0, _p(g), _p(b), eps, _p(post_mask), _p(out_f32),
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
    _req_opt(bias=bias, pre_scale=pre_scale, pre_mask=pre_mask, residual=residual, post_mask=post_mask)
    out = torch.empty(n_rows, n_out, device=x.device, dtype=torch.float32) if out is None else out
    _req(out, name="out")
    g, b, eps = _ln_args(ln, "ln")
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_linear_f32(
        _p(x), x.shape[1], _p(wpk32), _p(bias), n_rows, k_in, n_out, tiles, _p(pre_scale), int(bool(relu)), _p(pre_mask), _p(residual),
        residual.shape[-1] if residual is not None else 0, _p(g), _p(b), eps, _p(post_mask), _p(out), out.shape[-1], out_col0,
        _stream()), flops=2 * n_rows * k_in * n_out), "s2s_node_linear_f32")
    return out


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
    _req_all(t_img=t_img, node_const=node_const, fa=fa, fb=fb)
    M, dev = n_samples * n_res, t_img.device
    if (t_img.numel() not in (512, 512 * n_samples) or node_const.numel() not in (M * 256, n_res * 256) or fa.numel() != M * 128
            or fb.numel() != M * 128):
        raise HipLibraryError("embed_assemble: bad shapes")
    h = xp_alloc(M, 256, dev) if planes else torch.empty(M, 256, device=dev, dtype=torch.float32)
    node_a, node_b = torch.empty(n_samples, n_res, 128, device=dev, dtype=torch.float32), torch.empty_like(fb)
    _check(lib.s2s_embed_assemble(_p(t_img), t_img.numel() // 512 if t_img.numel() != 512 else 1, _p(node_const), node_const.numel() // 256,
                                  _p(fa), _p(fb), M, n_res, _p(h) if planes else None, None if planes else _p(h), _p(node_a), _p(node_b),
                                  int(b_col_blocked), _p(range_flag()), _stream()), "s2s_embed_assemble")
    return h, node_a, node_b


def row_layernorm(x, n_rows: int, n_cols: int, gamma, beta, eps: float, post_mask=None, out_f32=None, out_col0: int = 0, want_f32=True,
                  out_xp=None, out_xp_k: Optional[int] = None, out_xp_k0: int = 0, want_xp=False):
    """LayerNorm (+ post mask) of the leading ``n_cols`` columns of fp32 rows with the node GEMM's epilogue code (s2s_row_layernorm):
    the second half of a layer whose GEMM ran without its LayerNorm.  Same output conventions as ``node_linear``."""
    lib = load_library()
    _req(x, name="x"); _req(gamma, name="ln.gamma"); _req(beta, name="ln.beta")
    _req_opt(post_mask=post_mask)
    out_f32, out_xp, out_xp_k = _node_outputs(n_rows, n_cols, x.device, out_f32, want_f32, out_xp, out_xp_k, want_xp)
    _check(_timed("s2s_node_linear", lambda: lib.s2s_row_layernorm(
        _p(x), x.shape[-1], n_rows, n_cols, _p(gamma), _p(beta), float(eps), _p(post_mask), _p(out_f32),
        out_f32.shape[-1] if out_f32 is not None else 0, out_col0, _p(out_xp), (out_xp_k or 0) // 16, out_xp_k0 // 16, _p(range_flag()),
        _stream())), "s2s_row_layernorm")
    return out_f32, out_xp


def node_apply(x, layer: dict, n_rows: int, *, out_f32=None, out_col0: int = 0, want_f32=True, out_xp=None, out_xp_k=None,
               out_xp_k0: int = 0, want_xp=False, **epilogue):
    """One layer of the node stream in the arithmetic of its INPUT: ``x`` packed f16 planes (int16) -> s2s_node_linear, ``x`` fp32
    [n_rows, K] -> s2s_node_linear_f32.  ``layer`` = pack_node_layer(...).  Same calling convention and return value
    (fp32 output or None, activation-format output or None) in both; in the fp32 arithmetic the two outputs are the same tensor
    (``out_xp``, an fp32 buffer there, is written at column ``out_xp_k0`` when no ``out_f32`` is given)."""
    T = torch.ops.str2str_amd
    ep = dict(epilogue)
    g, b, eps = _ln_args(ep.pop("ln", None))
    row_map = ep.pop("row_map", None)
    flat = (ep.pop("pre_scale", None), bool(ep.pop("relu", False)), ep.pop("pre_mask", None), ep.pop("residual", None), g, b, eps,
            ep.pop("post_mask", None))
    outs = (out_f32, out_col0, want_f32, out_xp, _int_arg(out_xp_k), out_xp_k0, want_xp)
    if ep:
        raise TypeError(f"node_apply: unexpected arguments {sorted(ep)}")
    if x.dtype == torch.int16 and g is not None and n_rows <= SMALL_ROWS and layer["k"] >= 1024 and layer["n"] in (256, 320) and row_map is None:
        # a long contraction on few rows whose epilogue normalises over the row (linear_out, K = 2688): one column block per row tile
        # is K / 16 serial k-steps of 24 MFMAs on 1 / 6 of the chip; GEMM in narrow blocks + the LayerNorm on its own is the same
        # arithmetic (s2s_row_layernorm) in a third of the time
        pre = torch.empty(n_rows, layer["n"], device=x.device, dtype=torch.float32)
        T.node_linear(x, layer["w_n"], layer["b"], n_rows, layer["k"], layer["n"], 2, *flat[:4], None, None, 0.0, None, pre)
        return T.row_layernorm(pre, n_rows, layer["n"], g, b, eps, flat[7], *outs)
    if x.dtype == torch.int16:
        mp, ms = row_map if row_map is not None else (0, 0)
        wk, tg = small_rows_variant(layer, n_rows)
        return T.node_linear(x, layer[wk], layer["b"], n_rows, layer["k"], layer["n"], tg, *flat, *outs, mp, ms)
    if row_map is not None:
        raise HipLibraryError("node_apply: the row map belongs to the f16 attention operands")
    if out_f32 is not None and out_xp is not None and out_xp is not out_f32:
        raise HipLibraryError("node_apply (fp32): one output buffer")
    out, col0 = (out_f32, out_col0) if out_f32 is not None else (out_xp, out_xp_k0)
    y = T.node_linear_f32(x, layer["w32"], layer["b"], n_rows, layer["k"], layer["n"], layer["tg"], *flat, out, col0)
    return y, y


def node_linear_vfrag(xp, wpk, bias, n_rows: int, k_in: int, n_out: int, tiles_per_head: int = 8, out=None, row_map: Optional[tuple] = None):
    """Projection stored as MFMA A fragments of f16 pairs over 32-row tiles (s2s_node_linear_vfrag; the value projection of the IPA).
    -> int16 buffer [row tiles][heads][tiles_per_head][2][2][64][8]."""
    lib = load_library()
    _req(xp, torch.int16, "xp"); _req(wpk, torch.int16, "w_packed")
    _req_opt(bias=bias)
    out = _req(vf_alloc(n_rows, n_out, xp.device) if out is None else out, torch.int16, "out_vf")
    map_pad, map_src = row_map if row_map is not None else (0, 0)
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_linear_vfrag(_p(xp), _p(wpk), _p(bias), n_rows, k_in, n_out, tiles_per_head,
                                                                       _p(out), map_pad, map_src, _p(range_flag()), _stream()),
                  flops=2 * n_rows * k_in * n_out), "s2s_node_linear_vfrag")
    return out


class _NodeProblem(ctypes.Structure):   # s2s_node_problem (include/str2str_hip.h)
    _fields_ = [("xp", ctypes.c_void_p), ("w_packed", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("n_rows", ctypes.c_longlong),
                ("k_in", ctypes.c_int), ("n_out", ctypes.c_int), ("tiles_per_block", ctypes.c_int), ("vfrag_tiles_per_head", ctypes.c_int),
                ("out_f32", ctypes.c_void_p), ("out_ld", ctypes.c_int), ("out_col0", ctypes.c_int), ("out_xp", ctypes.c_void_p),
                ("out_xp_ksteps", ctypes.c_int), ("out_xp_kstep0", ctypes.c_int), ("out_vf", ctypes.c_void_p), ("map_pad", ctypes.c_int),
                ("map_src", ctypes.c_int), ("relu", ctypes.c_int), ("pre_scale", ctypes.c_void_p)]


def _fill_problem(p, xp, w, bias, n_rows, k_in, n_out, tiles, **fields):
    """One s2s_node_problem: the operands every problem has, then whatever it sets of outputs, row map, relu and pre-scale."""
    p.xp, p.w_packed, p.bias = xp.data_ptr(), w.data_ptr(), bias.data_ptr()
    p.n_rows, p.k_in, p.n_out, p.tiles_per_block = n_rows, k_in, n_out, tiles
    for name, val in fields.items():
        setattr(p, name, val)


def _launch_problems(lib, arr, n):
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_linear_multi(ctypes.byref(arr), n, _p(range_flag()), _stream()),
                  flops=sum(2 * arr[i].n_rows * arr[i].k_in * arr[i].n_out for i in range(n))), "s2s_node_linear_multi")


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
        fields = {"relu": relu}
        if pre_scale[i].numel():
            fields.update(pre_scale=_req(pre_scale[i], name="pre_scale").data_ptr())
        if out_f32[i].numel():
            fields.update(out_f32=_req(out_f32[i], name="out_f32").data_ptr(), out_ld=ld, out_col0=c0)
        if out_xp[i].numel():
            fields.update(out_xp=_req(out_xp[i], torch.int16, "out_xp").data_ptr(), out_xp_ksteps=xk // 16, out_xp_kstep0=xk0 // 16)
        _fill_problem(arr[i], xp, _req(w[i], torch.int16, "w"), _req(bias[i], name="bias"), rows, k, nn, tg, **fields)
    _launch_problems(lib, arr, n)


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
    v_vf = vf_alloc(n_rows_padded, v["n"], dev) if v is not None else None
    qp_o = torch.empty(n_rows, qp["n"], device=dev, dtype=torch.float32)
    kvp_o = torch.empty(n_rows, kvp["n"], device=dev, dtype=torch.float32)
    problems = [(q, n_rows_padded, dict(out_xp=q_xp.data_ptr(), out_xp_ksteps=q["n"] // 16, map_pad=mp, map_src=ms))]
    if k is not None:
        problems.append((k, n_rows_padded, dict(out_xp=k_xp.data_ptr(), out_xp_ksteps=k["n"] // 16, map_pad=mp, map_src=ms)))
    if v is not None:
        problems.append((v, n_rows_padded, dict(vfrag_tiles_per_head=tiles_per_head, out_vf=v_vf.data_ptr(), map_pad=mp, map_src=ms)))
    problems += [(qp, n_rows, dict(out_f32=qp_o.data_ptr(), out_ld=qp["n"])), (kvp, n_rows, dict(out_f32=kvp_o.data_ptr(), out_ld=kvp["n"]))]
    arr = (_NodeProblem * len(problems))()
    for p, (layer, rows, fields) in zip(arr, problems):   # (the caller picked the variant: "w" / "tg")
        _fill_problem(p, s_xp, layer["w"], layer["b"], rows, layer["k"], layer["n"], layer["tg"], **fields)
    _launch_problems(lib, arr, len(problems))
    return q_xp, k_xp, v_vf, qp_o, kvp_o


class _ChainLayer(ctypes.Structure):   # s2s_chain_layer (include/str2str_hip.h)
    _fields_ = [("w_packed", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("relu", ctypes.c_int)]


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
    mg, mb, meps = _ln_args(mid_ln, "mid_ln")
    k0 = width if k_in0 is None else int(k_in0)
    if n not in (2, 3, 4) or len(bias) != n or len(relu) != n or width not in CHAIN_WIDTHS or (k0 != width and (width, k0) != (256, 320)):
        raise HipLibraryError("node_chain: 2 .. 4 layers of width 256 or 320 (first layer: 320 -> 256 allowed)")
    arr = (_ChainLayer * n)()
    for i in range(n):
        _req(w_row[i], torch.int16, "w_row"); _req(bias[i], name="bias")
        if w_row[i].numel() != width * (k0 if i == 0 else width) * 2 or bias[i].numel() < width:
            raise HipLibraryError("node_chain: weights must be packed with one column block of the layer's width")
        arr[i].w_packed, arr[i].bias, arr[i].relu = w_row[i].data_ptr(), bias[i].data_ptr(), int(bool(relu[i]))
    _req_opt(pre_mask=pre_mask, residual=residual, ln_gamma=ln_gamma, ln_beta=ln_beta, post_mask=post_mask, mid_residual=mid_residual,
             mid_out_f32=mid_out_f32)
    out_f32, out_xp, out_xp_k = _node_outputs(n_rows, width, xp.device, out_f32, want_f32, out_xp, out_xp_k, want_xp)
    _check(_timed("s2s_node_linear", lambda: lib.s2s_node_chain(
        _p(xp), ctypes.byref(arr), n, n_rows, width, k0, _p(mid_residual), mid_residual.shape[-1] if mid_residual is not None else 0,
        _p(mid_out_f32), mid_out_f32.shape[-1] if mid_out_f32 is not None else 0, _p(mg), _p(mb), meps, _p(pre_mask), _p(residual),
        residual.shape[-1] if residual is not None else 0, _p(ln_gamma), _p(ln_beta), float(ln_eps), _p(post_mask), _p(out_f32),
        out_f32.shape[-1] if out_f32 is not None else 0, out_col0, _p(out_xp), (out_xp_k or 0) // 16, out_xp_k0 // 16, _p(range_flag()),
        _stream()), flops=2 * n_rows * width * (k0 + (n - 1) * width)), "s2s_node_chain")
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
    return torch.ops.str2str_amd.node_chain(x, [L["w_row"] for L in layers], [L["b"] for L in layers], [bool(r) for r in relu], n_rows, width,
                                            kw.get("pre_mask"), kw.get("residual"), *_ln_args(kw.get("ln")), kw.get("post_mask"),
                                            kw.get("out_f32"), kw.get("out_col0", 0), kw.get("want_f32", True), kw.get("out_xp"),
                                            _int_arg(kw.get("out_xp_k")), kw.get("out_xp_k0", 0), kw.get("want_xp", False), k0, first_res,
                                            first_out, *_ln_args(first_ln))


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
        o32, oxp, xk = _node_outputs(n_rows, layer["n"], dev, kw.get("out_f32"), kw.get("want_f32", True), kw.get("out_xp"),
                                     kw.get("out_xp_k"), kw.get("want_xp", False))
        w.append(layer[key]); bias.append(layer["b"]); ps.append(kw["pre_scale"] if kw.get("pre_scale") is not None else empty_f)
        dims += [n_rows, layer["k"], layer["n"], tg, o32.shape[-1] if o32 is not None else 0, kw.get("out_col0", 0), xk or 0,
                 kw.get("out_xp_k0", 0), int(bool(kw.get("relu", False)))]
        of.append(o32 if o32 is not None else empty_f); ox.append(oxp if oxp is not None else empty_i)
        res.append((o32, oxp))
    torch.ops.str2str_amd.node_linear_multi(x, w, bias, ps, dims, of, ox)
    return res
