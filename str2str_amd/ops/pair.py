"""Pair stream: edge transition, edge embedding and the pair projection of an IPA block."""
import torch

from .binding import HipLibraryError, _check, _p, _req, _req_all, _req_opt, _stream, _timed, load_library
from .packing import PairByClass, PairTiled, column_blocked
from .range_guard import range_flag


def _proj_outputs(proj, B, N, dev, dtype=torch.float32, name="proj.wp"):
    """``proj`` = (weights, bias64) of the next IPA block, fused into a pair kernel -> (weights, bias64, attn_bias [B,8,N,N] (head-major),
    pair_z [B,N,N,32]) with the two outputs allocated here, or four Nones."""
    if proj is None:
        return None, None, None, None
    w, b64 = proj
    _req(w, dtype, name); _req(b64, name="proj.b64")
    return w, b64, torch.empty(B, 8, N, N, device=dev, dtype=torch.float32), torch.empty(B, N, N, 32, device=dev, dtype=torch.float32)


def edge_transition_f16x3(edge, node_ab, node_p, wstream, b2, gamma, beta, mask, ln_eps=1e-5, out=None, proj=None,
                          out_layout: str = "rowmajor", prescale_exp: int = 0, ab_kernel_form: bool = False):
    """EdgeTransition on split-f16 MFMA (fp32-equivalent accuracy; csrc/edge_transition_f16.h); same contract as ``edge_transition``.
    ``proj`` = (31-stage stream = this layer's 30 stages (``pack_f16x3_stream``) + the next IPA block's projection stage
    (``pack_f16x2_layer``), bias64) also returns that block's (attn_bias [B,8,N,N], pair_z [B,N,N,32]).
    ``edge`` may be a ``PairTiled``, or a ``PairByClass`` (the edge embedding's class table + one class index per pair: the kernel reads
    each pair's row out of the table; only with ``proj``); ``out_layout``: "rowmajor" (the reference's tensor), "tiled" (-> ``PairTiled``) or "none" (the pair
    vectors are not written: only with ``proj``, for the last EdgeTransition of a trunk; returns None in their place).
    ``prescale_exp`` = e (0 .. 15): the kernel keeps its hidden activations as f16 planes of 2^-e x the value (a block exponent: exact,
    same speed) -- what the sampler sets when the range guard reports hidden activations of 2^15 and beyond.
    ``node_ab`` [B,N,896] = [W1[:,128:256] n' + b1 | W1[:,256:] n' | Wf[:,256:] n' + bf] as ``EdgeTransition.node_parts`` gives it (the
    pair's per-node linear parts: row half and column half of the first layer, the j-side residual taken through the final layer incl.
    its bias); ``ab_kernel_form``: the column half and the third group already carry the accumulators' 2^5 (the trunk's per-node layers
    produce them so: no extra launch), see the C header.  A plain ``node_ab``'s third group is centred over its 128 channels here (the
    LayerNorm removes a common component anyway, and as the accumulators' start value it would cost every accumulation its
    rounding); the kernel form must arrive centred, as ``EdgeTransition.node_layers`` produces it."""
    lib = load_library()
    B, N = edge.shape[0], edge.shape[1]
    in_tiled, in_cls = isinstance(edge, PairTiled), isinstance(edge, PairByClass)
    if in_cls and proj is None:
        raise HipLibraryError("edge_transition_f16x3: a PairByClass input needs the fused projection (proj); pair_untiled materialises it")
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
        if not ab_kernel_form:
            # G_j starts the final layer's accumulators, in front of the LayerNorm: a component common to its 128 channels would only
            # cost every accumulation its rounding.  Given vectors are centred here; the kernel form arrives centred (EdgeTransition.node_layers)
            node_ab[..., 768:] -= node_ab[..., 768:].mean(dim=-1, keepdim=True)
    if out_layout not in ("rowmajor", "tiled", "none") or (out_layout == "none" and proj is None):
        raise HipLibraryError(f"edge_transition_f16x3: out_layout {out_layout!r}" + (" needs proj" if out_layout == "none" else ""))
    _req(edge.buf if in_tiled or in_cls else edge, name="edge")
    _req_all(node_ab=node_ab, node_p=node_p, b2=b2, gamma=gamma, beta=beta)
    pw, pb, pbias, ppz = _proj_outputs(proj, B, N, edge.device, torch.int16, "wstream")
    wstream = _req(wstream, torch.int16, "wstream") if proj is None else pw
    if wstream.numel() * 2 != (31 if proj is not None else 30) * 32 * 1024:
        raise HipLibraryError("edge_transition_f16x3: weight stream has the wrong number of stages")
    _req_opt(mask=mask)
    if out_layout == "none":
        out = None
    elif out is None:
        out = PairTiled(B, N, edge.device) if out_layout == "tiled" else torch.empty(B, N, N, 128, device=edge.device, dtype=torch.float32)
    elif out.data_ptr() == edge.data_ptr():
        raise HipLibraryError("edge_transition: out may not alias edge")
    elif isinstance(out, PairTiled) != (out_layout == "tiled"):
        raise HipLibraryError("edge_transition_f16x3: out does not have the requested layout")
    io = (1 if in_tiled else 0) | {"rowmajor": 0, "tiled": 2, "none": 4}[out_layout] | ((8 | (16 if edge.rec == 168 else 0)) if in_cls else 0)
    _check(_timed("s2s_edge_transition", lambda: lib.s2s_edge_transition_f16x3(
        _p(edge.buf if in_tiled or in_cls else edge), _p(node_ab), _p(node_p), _p(wstream), _p(b2), _p(gamma), _p(beta), _p(mask),
        _p(out.buf if isinstance(out, PairTiled) else out), B, N, ln_eps, io, _p(pb), _p(pbias), _p(ppz), int(prescale_exp), _p(range_flag()),
        _stream())), "s2s_edge_transition_f16x3")
    return out if proj is None else (out, pbias, ppz)


def edge_transition(edge, node_ab, node_p, w1p, w2p, wfp, b2, bf, gamma, beta, mask, ln_eps=1e-5, out=None, proj=None):
    """-> out, or (out, attn_bias, pair_z) when ``proj`` = (packed Wcat, bias64) of the next IPA block is given."""
    lib = load_library()
    B, N = edge.shape[0], edge.shape[1]
    _req(edge, name="edge")
    if edge.shape != (B, N, N, 128) or node_ab.shape != (B, N, 768) or node_p.shape != (B, N, 128):
        raise HipLibraryError(f"edge_transition: bad shapes {tuple(edge.shape)} {tuple(node_ab.shape)} {tuple(node_p.shape)}")
    _req_all(node_ab=node_ab, node_p=node_p, w1p=w1p, w2p=w2p, wfp=wfp, b2=b2, bf=bf, gamma=gamma, beta=beta)
    _req_opt(mask=mask)
    if out is None:
        out = torch.empty_like(edge)
    elif out.data_ptr() == edge.data_ptr():
        raise HipLibraryError("edge_transition: out may not alias edge")
    _req(out, name="out")
    pw, pb, pbias, ppz = _proj_outputs(proj, B, N, edge.device)
    _check(_timed("s2s_edge_transition", lambda: lib.s2s_edge_transition(
        _p(edge), _p(node_ab), _p(node_p), _p(w1p), _p(w2p), _p(wfp), _p(b2), _p(bf), _p(gamma), _p(beta), _p(mask),
        _p(out), B, N, ln_eps, _p(pw), _p(pb), _p(pbias), _p(ppz), _stream())), "s2s_edge_transition")
    return out if proj is None else (out, pbias, ppz)


def edge_embed(node_a, node_b, rel_table, bin_table, bin_lower, residue_idx, ca, w2p, w3p, b2, b3, gamma, beta, mask,
               rel_offset: int, ln_eps=1e-5, out=None, proj=None):
    lib = load_library()
    B, N = node_a.shape[0], node_a.shape[1]
    _req_all(node_a=node_a, node_b=node_b, rel_table=rel_table, bin_table=bin_table, bin_lower=bin_lower, ca=ca, w2p=w2p, w3p=w3p, b2=b2, b3=b3,
             gamma=gamma, beta=beta)
    _req(residue_idx, torch.int64, "residue_idx")
    _req_opt(mask=mask)
    out = torch.empty(B, N, N, 128, device=node_a.device, dtype=torch.float32) if out is None else out
    pw, pb, pbias, ppz = _proj_outputs(proj, B, N, node_a.device)
    _check(lib.s2s_edge_embed(_p(node_a), _p(node_b), _p(rel_table), _p(bin_table), _p(bin_lower), _p(residue_idx), _p(ca),
                              _p(w2p), _p(w3p), _p(b2), _p(b3), _p(gamma), _p(beta), _p(mask), _p(out), B, N,
                              int(rel_offset), rel_table.shape[0], bin_table.shape[0], ln_eps, _p(pw), _p(pb), _p(pbias),
                              _p(ppz), _stream()), "s2s_edge_embed")
    return out if proj is None else (out, pbias, ppz)


def edge_embed_f16x3(node_a, node_b, rel_table, bin_table, bin_lower, residue_idx, ca, wstream, b2, b3, gamma, beta, mask,
                     rel_offset: int, ln_eps=1e-5, out=None, proj=None, column_blocked_tables=False, out_layout: str = "rowmajor"):
    """Edge embedding on split-f16 MFMA (csrc/edge_embed_f16.h); ``proj`` = (5-stage stream, bias64) also returns (attn_bias, pair_z).
    node_b / rel_table / bin_table: [.., rows, 128], or already ``column_blocked`` ([.., 32, rows, 4]) with the flag set.
    ``out_layout`` "tiled" -> a ``PairTiled`` for ``edge_transition_f16x3``."""
    lib = load_library()
    B, N = node_a.shape[0], node_a.shape[1]
    if not column_blocked_tables:
        node_b, rel_table, bin_table = column_blocked(node_b), column_blocked(rel_table), column_blocked(bin_table)
    if node_b.shape != (B, 32, N, 4) or rel_table.shape[0] != 32 or bin_table.shape[0] != 32:
        raise HipLibraryError("edge_embed_f16x3: tables are not column-blocked [.., 32, rows, 4]")
    _req_all(node_a=node_a, node_b=node_b, rel_table=rel_table, bin_table=bin_table, bin_lower=bin_lower, ca=ca, b2=b2, b3=b3, gamma=gamma, beta=beta)
    _req(residue_idx, torch.int64, "residue_idx")
    pw, pb, pbias, ppz = _proj_outputs(proj, B, N, node_a.device, torch.int16, "wstream")
    wstream = _req(wstream, torch.int16, "wstream") if proj is None else pw
    if wstream.numel() * 2 != (5 if proj is not None else 4) * 32 * 1024:
        raise HipLibraryError("s2s_edge_embed_f16x3: weight stream has the wrong number of stages")
    _req_opt(mask=mask)
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


# ---- the edge embedding by class (s2s_edge_embed_classes_f16x3 + s2s_edge_embed_expand; include/str2str_hip.h)
# R of the eligibility rule  class rows x R <= B N^2.  Per row the table kernel costs what the edge embedding costs per pair, and the
# two launches cost a few microseconds more than one, so the path can only win where the table is a small fraction of the pairs.
# Set from the measured crossover with a factor 2 on the old kernel's side: profiles/r07_ee_classes_threshold.md.
EE_CLASS_R = 12


def edge_embed_class_rows(n_fixed: int, n_rel: int, n_bins: int) -> int:
    """Rows of the class table: every (fa, fb) of the fixed-mask values present x every relative-position row x (no bin | each bin)."""
    if n_fixed not in (1, 2):
        raise HipLibraryError(f"edge_embed classes: {n_fixed} fixed-mask values (a 0/1 mask has one or two)")
    return (4 if n_fixed == 2 else 1) * n_rel * (n_bins + 1)


def edge_embed_class_row(fa: int, fb: int, d: int, bin_: int, n_rel: int, n_bins: int) -> int:
    """Row of class (fa, fb, d, bin), bin = -1 for "none" (csrc/edge_embed_class.h: ee_class_row)."""
    return ((fa * 2 + fb) * n_rel + d) * (n_bins + 1) + (bin_ + 1)


def edge_embed_class_of_row(r: int, n_rel: int, n_bins: int):
    """Inverse of ``edge_embed_class_row`` (the table kernel's decode) -> (fa, fb, d, bin)."""
    q, b1 = divmod(r, n_bins + 1)
    c, d = divmod(q, n_rel)
    return c >> 1, c & 1, d, b1 - 1


def edge_embed_classes_eligible(mode: str, arith: str, one_timestep: bool, n_fixed, mask_is_01: bool, n_rel: int, n_bins: int,
                                B: int, N: int, R: int = EE_CLASS_R) -> bool:
    """Whether a call of the edge embedding takes the class path.  ``mode`` = S2S_EE_CLASSES: "0" never, "1" whenever it is legal,
    "auto" when it is legal and the table is small against the work.  Legal: f16x3 arithmetic, one timestep for the chunk, a fixed
    mask that is exactly 0/1 (``n_fixed`` = how many of the two values occur, None if it is not) and a node mask that is 0/1 or absent."""
    if mode not in ("auto", "0", "1"):
        raise ValueError(f"S2S_EE_CLASSES={mode!r}: expected auto, 0 or 1")
    if mode == "0" or arith != "f16x3" or not one_timestep or n_fixed not in (1, 2) or not mask_is_01:
        return False
    rows = edge_embed_class_rows(n_fixed, n_rel, n_bins)
    if rows * 168 * 4 >= 2 ** 32:    # the table kernel's 32-bit offsets
        return False
    return mode == "1" or rows * R <= B * N * N


def edge_embed_classes_f16x3(node_a2, node_b2, fixed_cls, rel_table, bin_table, bin_lower, residue_idx, ca, wstream, b2, b3, gamma, beta,
                             mask, rel_offset: int, ln_eps=1e-5, out=None, proj=None, out_layout: str = "rowmajor"):
    """The edge embedding by class: ``edge_embed_f16x3``'s outputs (same return contract, bit for bit where the edge mask is non-zero)
    for a chunk that shares one timestep and has a 0/1 fixed mask and node mask -- the MLP once per class row, then a copy per pair.
    ``out_layout`` "by_class": the pair tensor is NOT materialised -- a ``PairByClass`` (the table and one class index per pair) for
    ``edge_transition_f16x3``; attn_bias and pair_z are written as in the other layouts.
    ``node_a2`` [n_fixed,128] / ``node_b2`` [32,n_fixed,4]: what ``embed_assemble`` gives for a pseudo-sample whose fixed mask runs over
    the n_fixed values present; ``fixed_cls`` [B,N] int32: each residue's index among them; tables column-blocked."""
    lib = load_library()
    B, N = fixed_cls.shape
    n_fixed, n_rel, n_bins = node_a2.numel() // 128, rel_table.shape[1], bin_table.shape[1]
    if node_b2.numel() != n_fixed * 128 or rel_table.shape[0] != 32 or bin_table.shape[0] != 32:
        raise HipLibraryError("edge_embed_classes_f16x3: operands are not [n_fixed,128] / column-blocked [32, rows, 4]")
    rows = edge_embed_class_rows(n_fixed, n_rel, n_bins)
    _req_all(node_a2=node_a2, node_b2=node_b2, rel_table=rel_table, bin_table=bin_table, bin_lower=bin_lower, ca=ca, b2=b2, b3=b3, gamma=gamma,
             beta=beta)
    _req(residue_idx, torch.int64, "residue_idx"); _req(fixed_cls, torch.int32, "fixed_cls")
    if tuple(residue_idx.shape) != (B, N) or ca.numel() != B * N * 3:
        raise HipLibraryError("edge_embed_classes_f16x3: residue_idx / ca do not match fixed_cls [B, N]")
    dev = node_a2.device
    pw, pb, pbias, ppz = _proj_outputs(proj, B, N, dev, torch.int16, "wstream")
    wstream = _req(wstream, torch.int16, "wstream") if proj is None else pw
    if wstream.numel() * 2 != (5 if proj is not None else 4) * 32 * 1024:
        raise HipLibraryError("s2s_edge_embed_classes_f16x3: weight stream has the wrong number of stages")
    _req_opt(mask=mask)
    if out_layout not in ("rowmajor", "tiled", "by_class") or (out_layout == "by_class" and out is not None):
        raise HipLibraryError(f"edge_embed_classes_f16x3: out_layout {out_layout!r}" + (" takes no out" if out is not None else ""))
    by_cls = out_layout == "by_class"

    def pair_out(out, tiled):   # the materialised pair tensor of an expansion
        if out is None:
            out = PairTiled(B, N, dev) if tiled else torch.empty(B, N, N, 128, device=dev, dtype=torch.float32)
        elif isinstance(out, PairTiled) != tiled:
            raise HipLibraryError("edge_embed_classes_f16x3: out does not have the requested layout")
        return out

    def expand(z, mode, pbias, ppz):   # mode: s2s_edge_embed_expand's out_tiled (0 row-major, 1 tiled, 2 class indices)
        return lib.s2s_edge_embed_expand(_p(table), _p(fixed_cls), _p(bin_lower), _p(residue_idx), _p(ca), _p(mask), _p(pb), _p(z), mode,
                                         _p(pbias), _p(ppz), B, N, int(rel_offset), n_rel, n_bins, _stream())

    if not by_cls:
        out = pair_out(out, out_layout == "tiled")
    # one buffer [M32 index words | zero record | table] by class (``PairByClass``), the table alone (M32 = 0, no zero record) otherwise
    rec, m32 = 168 if proj is not None else 128, PairByClass.index_words(B, N) if by_cls else 0
    buf = torch.empty(m32 + (rows + (1 if by_cls else 0)) * rec, device=dev, dtype=torch.float32)
    table = buf[m32 + (rec if by_cls else 0):].view(rows, rec)

    def launch():   # both launches under one timer: the family's time is the table plus the expansion
        rc = lib.s2s_edge_embed_classes_f16x3(_p(node_a2), _p(node_b2), _p(rel_table), _p(bin_table), _p(wstream), _p(b2), _p(b3), _p(gamma),
                                              _p(beta), _p(table), n_fixed, n_rel, n_bins, ln_eps, _p(pb), _p(range_flag()), _stream())
        if by_cls:
            buf[m32:m32 + rec].zero_()   # the zero record: what a masked pair's index + 1 points at
        return rc or (expand(buf, 2, pbias, ppz) if by_cls else expand(out.buf if out_layout == "tiled" else out, 1 if out_layout == "tiled" else 0, pbias, ppz))

    _check(_timed("s2s_edge_embed", launch), "s2s_edge_embed_classes_f16x3 / s2s_edge_embed_expand")
    if by_cls:
        def materialise():   # the row-major tensor from the same table: z alone (the record size follows from the bias pointer)
            z = pair_out(None, False)
            _check(expand(z, 0, None, None), "s2s_edge_embed_expand")
            return z
        out = PairByClass(B, N, buf, rec, expand=materialise)
    return out if proj is None else (out, pbias, ppz)


def pair_project(edge, wp, bias64, attn_bias=None, pair_z=None):
    lib = load_library()
    B, N = edge.shape[0], edge.shape[1]
    _req(edge, name="edge"); _req(wp, name="wp"); _req(bias64, name="bias64")
    attn_bias = torch.empty(B, 8, N, N, device=edge.device, dtype=torch.float32) if attn_bias is None else attn_bias  # head-major [B,H,N,N]
    pair_z = torch.empty(B, N, N, 32, device=edge.device, dtype=torch.float32) if pair_z is None else pair_z
    _check(lib.s2s_pair_project(_p(edge), _p(wp), _p(bias64), _p(attn_bias), _p(pair_z), B, N, _stream()), "s2s_pair_project")
    return attn_bias, pair_z
