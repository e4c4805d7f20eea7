"""Weight packers and layout converters: plain torch, no library and no GPU needed."""
from typing import Optional

import torch

from .binding import HipLibraryError, WeightRangeError


def _pad_rows32(w: torch.Tensor) -> torch.Tensor:
    """[n_out, k] with n_out zero-padded to a multiple of 32 (whole output tiles)."""
    pad = (-w.shape[0]) % 32
    return torch.cat([w, w.new_zeros(pad, w.shape[1])], dim=0) if pad else w


def pack_weight(w: torch.Tensor, tile_major: bool = False) -> torch.Tensor:
    """[Mout, K] row-major -> kernel lane order (see include/str2str_hip.h).  Mout is zero-padded to
    a multiple of 32; K must be a multiple of 8.  ``tile_major`` orders fragments [t][s4] (a whole output
    tile is contiguous; s2s_edge_transition) instead of [s4][t]."""
    k = w.shape[1]
    if k % 8:
        raise ValueError("K must be a multiple of 8")
    w = _pad_rows32(w)
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
    the power of two keeps W_l in f16's normal range; the kernels take 2^-5 back in their epilogues (csrc/pair_f16.h).
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
    8 slots = one 32 KiB stage, 30 stages) in the kernel's consumption order (csrc/edge_transition_f16.h):
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


class PairByClass:
    """The edge embedding's [B,N,N,128] pair tensor BY CLASS (include/str2str_hip.h, "Pair-tensor layouts"): not materialised, but one
    flat fp32 buffer  [M32 int32 words: each pair's class row, -1 where the edge mask is zero | a zero record | the class table's records
    of ``rec`` floats, z[128] first],  M32 = B N N rounded up to 32.  ``ops.edge_embed_classes_f16x3(out_layout="by_class")`` makes one
    and the first ``edge_transition_f16x3`` reads it; ``expand`` (set by the producer) materialises the row-major tensor through the
    expansion kernel for every other reader (``pair_untiled``)."""
    __slots__ = ("buf", "B", "N", "rec", "expand")

    def __init__(self, B: int, N: int, buf: torch.Tensor, rec: int, expand=None):
        self.B, self.N, self.rec, self.buf, self.expand = int(B), int(N), int(rec), buf, expand
        if self.rec not in (128, 168) or buf.dtype != torch.float32 or buf.ndim != 1 or not buf.is_contiguous() or (buf.numel() - self.M32) % self.rec:
            raise HipLibraryError("PairByClass: buffer must be a flat contiguous fp32 tensor of M32 index words and records of 128 or 168 floats")

    @staticmethod
    def index_words(B: int, N: int) -> int:
        """M32: the words in front of the records (one per pair, rounded up to 32: the records start 16-byte aligned)."""
        return -(-(int(B) * int(N) * int(N)) // 32) * 32

    M32 = property(lambda self: self.index_words(self.B, self.N))
    shape = property(lambda self: (self.B, self.N, self.N, 128))
    device = property(lambda self: self.buf.device)
    is_cuda = property(lambda self: self.buf.is_cuda)
    index = property(lambda self: self.buf[:self.B * self.N * self.N].view(torch.int32).view(self.B, self.N, self.N))   # class row or -1
    records = property(lambda self: self.buf[self.M32:].view(-1, self.rec))                                             # record 0 = zeros, class r = record r + 1

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


def pair_untiled(t) -> torch.Tensor:
    """``PairTiled`` -> row-major (plain torch), ``PairByClass`` -> row-major through the expansion kernel of its producer."""
    if isinstance(t, PairByClass):
        if t.expand is None:
            raise HipLibraryError("pair_untiled: this PairByClass does not come from edge_embed_classes_f16x3 (no expansion to materialise it with)")
        return t.expand()
    M = t.B * t.N * t.N
    return t.buf.view(-1, 16, 2, 32, 4).permute(0, 3, 1, 2, 4).reshape(-1, 128)[:M].reshape(t.B, t.N, t.N, 128).contiguous()


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


def padded_len(n_res: int) -> int:
    """n_res rounded up to the attention kernels' 32-residue tiles."""
    return (n_res + 31) // 32 * 32


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
    w, k = _pad_rows32(w), w.shape[1]
    if k % 32 or (w.shape[0] // 32) % tiles_per_block:
        raise ValueError("k_in must be a multiple of 32 and n_out/32 of tiles_per_block")
    fr = pack_f16x2_layer(w.float(), "chain")                       # [KS, T, 2, 64, 8]
    KS, T = fr.shape[:2]
    fr = fr.reshape(KS, T // tiles_per_block, tiles_per_block, 2, 64, 8).permute(1, 0, 2, 3, 4, 5)
    return fr.contiguous().view(torch.int16).reshape(-1)


def pack_node_weight_f32(w: torch.Tensor, tiles_per_block: int) -> torch.Tensor:
    """[n_out, k_in] fp32 -> fp32 blob [n_out/(32 TG)][k_in/8][TG][64][4] in the ``pack_weight`` lane order (s2s_node_linear_f32)."""
    w, k = _pad_rows32(w), w.shape[1]
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
    w = w.detach()

    def blocks(d, tiles):   # the f16 fragments in column blocks of ``tiles`` tiles (the default grouping's blob is shared)
        return d["w"] if tiles == tg else pack_node_weight(w.float(), tiles)

    # "w_row": one column block = the whole row (s2s_node_chain); "w_n": narrow blocks of two tiles (node_apply's GEMM + LayerNorm form)
    return LazyDict({"b": b.contiguous(), "n": n_pad, "k": k, "tg": tg, "tg_s": tg_s}, w=lambda d: pack_node_weight(w.float(), tg),
                    w_s=lambda d: blocks(d, tg_s), w_row=lambda d: blocks(d, t), w_n=lambda d: blocks(d, 2),
                    w32=lambda d: pack_node_weight_f32(w.float(), tg))


class LazyDict(dict):
    """dict whose named entries are built when first read (``lazy``: key -> builder, called with the dict)."""

    def __init__(self, eager: dict, **lazy):
        super().__init__(eager)
        self._lazy = lazy

    def __missing__(self, key):
        if key not in self._lazy:
            raise KeyError(key)
        self[key] = self._lazy[key](self)
        return self[key]


def xp_alloc(n_rows: int, k: int, device) -> torch.Tensor:
    """Packed-plane activation buffer for [n_rows, k] (int16 storage; two f16 planes per k-step; see include/str2str_hip.h)."""
    return torch.empty(((n_rows + 31) // 32) * (k // 16) * 2 * 64 * 8, dtype=torch.int16, device=device)


def vf_alloc(n_rows: int, n_out: int, device) -> torch.Tensor:
    """V-fragment buffer of an [n_rows, n_out] projection: int16 [row tiles][n_out / 32 tiles][2][2][64][8] (s2s_node_linear_vfrag)."""
    return torch.empty(((n_rows + 31) // 32) * (n_out // 32) * 2 * 2 * 64 * 8, dtype=torch.int16, device=device)


def act_alloc(n_rows: int, k: int, device, arith: str) -> torch.Tensor:
    """Activation buffer of the node stream: packed f16 planes ("f16x3") or fp32 row-major [n_rows, k] ("f32")."""
    return xp_alloc(n_rows, k, device) if arith == "f16x3" else torch.empty(n_rows, k, device=device, dtype=torch.float32)


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
