"""Seeded case table of the attention parity suite (tests/test_attention_parity.py, tests/test_attention_parity_cpu.py) and its
bound rule.

IPA inputs are those of ``InvariantPointAttention.attention(act, B, N, r7, mask, (attn_bias, pair_z))``: the node activation s
(masked, as the trunk hands it over), the head-major bias, pair_z, the frames and the residue mask.  Families:
  flat          today's amplitudes (s, bias, pair_z ~ N(0, 1)): the softmax is nearly uniform
  peaked        s x 3 and bias x 25 (+-50 at two sigma), plus in every third row +100 on one key of the LAST key tile and -100 on
                its neighbours: most rows put nearly all probability on one key, the logits of a row span more than float32's exp range, and the row
                maximum arrives in every key tile
  moved-flat    the same inputs with every frame of a sample under one random rotation and a translation of 10 scaled units
  moved-peaked  (100 A, the extent of ref64.se3_case); the operation is invariant, the kernels' arithmetic is not
Translations are a 0.38-unit chain walk (3.8 A CA-CA), centred per sample, except where moved.  Every sample of a batch has a
mask of another kind (MASK_KINDS), rotating over lengths and families.

Bound of a (family, section): 3 x the distance of the float32 chain (ref_attention in float32) from float64, pooled (max) over the
lengths of the family -- the kernels are that chain in another summation order; flat and moved-flat never more than the project's
5e-6.  Nothing here looks at a kernel.
"""
import functools
import math

import torch

import ref_attention as RA

LENGTHS = (1, 7, 32, 33, 64, 65, 96, 129, 257)
FAMILIES = ("flat", "peaked", "moved-flat", "moved-peaked")
# ones = the prefix of length N; last-tile = only the last key tile valid (rows whose earlier key tiles hold nothing but masked keys)
MASK_KINDS = ("ones", "gaps", "prefix-half", "tile1", "prefix-one", "first", "none", "last-tile")
H, C_S, C_PZ, TILE = 8, 256, 32, 32
S_PEAK, BIAS_PEAK, PLANT = 3.0, 25.0, 100.0
MOVE = 10.0
CAP = 5e-6


def base_family(family):
    return family[len("moved-"):] if family.startswith("moved-") else family


def mask_of(kind, N, g):
    m = torch.ones(N)
    if kind == "gaps":
        m = (torch.rand(N, generator=g) >= 0.3).float()
        m[int(torch.randint(N, (1,), generator=g))] = 1.0      # (never an empty sample by accident: "none" is the empty one)
    elif kind == "prefix-half":
        m[(N + 1) // 2:] = 0
    elif kind == "prefix-one":
        m[1:] = 0
    elif kind == "tile1":
        m[TILE:2 * TILE] = 0
    elif kind == "first":
        m[0] = 0
    elif kind == "none":
        m[:] = 0
    elif kind == "last-tile":
        m[:(N - 1) // TILE * TILE] = 0
    return m


def random_rotations(n, g, dtype=torch.float64):
    q = torch.randn(n, 4, generator=g, dtype=dtype)
    return q / q.norm(dim=-1, keepdim=True)


def quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def chain_walk(B, N, g):
    """Translations of a 0.38-unit random chain walk, centred per sample (float64)."""
    step = torch.randn(B, N, 3, generator=g, dtype=torch.float64)
    step = 0.38 * step / step.norm(dim=-1, keepdim=True)
    t = step.cumsum(dim=1)
    return t - t.mean(dim=1, keepdim=True)


def _build(family, B, N, seed, mask_offset):
    base = base_family(family)
    g = torch.Generator().manual_seed(seed)
    kinds = [MASK_KINDS[(mask_offset + b) % len(MASK_KINDS)] for b in range(B)]
    mask = torch.stack([mask_of(k, N, g) for k in kinds])
    s = torch.randn(B, N, C_S, generator=g)
    bias = torch.randn(B, H, N, N, generator=g)
    pz = torch.randn(B, N, N, C_PZ, generator=g)
    quat = random_rotations(B * N, g).view(B, N, 4)
    trans = chain_walk(B, N, g)
    if base == "peaked":
        s = s * S_PEAK
        bias = bias * BIAS_PEAK
        j0 = (N - 1) // TILE * TILE
        for i in range(0, N, 3):
            j = j0 + (i // 3) % (N - j0)
            for jj, v in ((j - 1, -PLANT), (j, PLANT), (j + 1, -PLANT)):
                if 0 <= jj < N:
                    bias[:, :, i, jj] = v
    s = s * mask[..., None]
    if family.startswith("moved-"):
        gm = torch.Generator().manual_seed(seed + 7919)
        rot = random_rotations(B, gm)                                           # one rigid motion per sample
        d = torch.randn(B, 3, generator=gm, dtype=torch.float64)
        d = MOVE * d / d.norm(dim=-1, keepdim=True)
        trans = torch.einsum("bij,bnj->bni", RA.quat_to_rot(rot), trans) + d[:, None, :]
        quat = quat_mul(rot[:, None, :], quat)
    r7_64 = torch.cat([quat, trans], dim=-1)
    return dict(name=f"{family}-B{B}-N{N}", family=family, B=B, N=N, s=s, bias=bias, pz=pz, r7_64=r7_64, r7=r7_64.float().contiguous(),
                mask=mask, kinds=kinds)


@functools.lru_cache(maxsize=None)
def case(family, N, B=3):
    """Case (family, N) of the table.  A moved case is its base case (same seed: same s, bias, pair_z, masks, local frames) moved."""
    k = LENGTHS.index(N) if N in LENGTHS else 0
    return _build(family, B, N, 5000 + 17 * N + (1 if base_family(family) == "peaked" else 0),
                  3 * k + 2 * FAMILIES.index(base_family(family)))


@functools.lru_cache(maxsize=None)
def many_items_case(family, N, B):
    """B samples of length N, every one with its own data and its own mask kind (B comes from the device's CU count)."""
    return _build(family, B, N, 9000 + N + (1 if base_family(family) == "peaked" else 0), 0)


def ipa_inputs(c, r7=None):
    return c["s"], c["bias"], c["pz"], (c["r7"] if r7 is None else r7), c["mask"]


# ---------------------------------------------------------------------------------------------------- the measure
def section_error(got, ref64, mask):
    """max |got - float64| / max(1, max |float64|) over the valid query rows of a section [B, N, cols] (nan if there is none)."""
    valid = mask.bool().to(ref64.device)
    if not bool(valid.any()):
        return float("nan")
    r = ref64[valid]
    return float((got.to(ref64.device).double()[valid] - r).abs().max() / max(1.0, float(r.abs().max())))


@functools.lru_cache(maxsize=None)
def _features(weights_key, family, N, B, dtype, many):
    c = many_items_case(family, N, B) if many else case(family, N, B)
    f = RA.ipa_features(_WEIGHTS[weights_key], *ipa_inputs(c), dtype=dtype)
    return {k: f[k] for k in RA.SECTIONS}


_WEIGHTS = {}


def register_weights(weights):
    """Weights (the block's tensors, ref_attention.ipa_weights) under a key that the caches can hash."""
    key = id(weights)
    _WEIGHTS[key] = weights
    return key


def features64(weights, c, many=False):
    """The float64 sections of a case of the table (evaluated once, shared by every test that needs them; do not modify)."""
    return _features(register_weights(weights), c["family"], c["N"], c["B"], torch.float64, many)


def chain_distance(weights, c):
    """{section: section_error of the float32 chain against float64} for a table case."""
    key = register_weights(weights)
    f32 = _features(key, c["family"], c["N"], c["B"], torch.float32, False)
    f64 = _features(key, c["family"], c["N"], c["B"], torch.float64, False)
    return {k: section_error(f32[k], f64[k], c["mask"]) for k in RA.SECTIONS}


@functools.lru_cache(maxsize=None)
def _pooled(weights_key, family):
    per = [chain_distance(_WEIGHTS[weights_key], case(family, N)) for N in LENGTHS]
    return {k: max(p[k] for p in per if not math.isnan(p[k])) for k in RA.SECTIONS}


def pooled_chain_distance(weights, family):
    return _pooled(register_weights(weights), family)


def bound(weights, family, section):
    rule = 3.0 * pooled_chain_distance(weights, family)[section]
    return min(rule, CAP) if base_family(family) == "flat" else rule


# ---------------------------------------------------------------------------------------------------- the encoder
ENC_LENGTHS = (1, 31, 33, 64, 65, 130, 257)
ENC_FAMILIES = ("flat", "peaked")
ENC_BIAS = ("none", "float-padding", "inf-prefix", "inf-first-tile")
ENC_B, ENC_HEADS, ENC_D = 3, 4, 320
ENC_PEAK = 4.0


@functools.lru_cache(maxsize=None)
def encoder_case(family, N, bias_kind):
    """qkv [B*N, 960] at the amplitude of an in_proj output (flat, N(0, 1)) or with q and k x 4 (peaked: one key takes nearly
    everything), where every even query row also carries a common vector u per head and the LAST key of the sample is u: for those
    rows the largest logit arrives in the last key tile, far above what came before, so the running maximum of an online softmax
    rises at the end and everything accumulated so far is rescaled.  key_bias: None | 0 / 1 float padding (added to the logits, as
    the reference does) | -inf beyond per-sample prefixes (N, about N / 2 -- whole trailing tiles masked --, 1) | -inf on the first
    key tile (N > 32; all but the last key otherwise).  Every row keeps at least one key."""
    B, D = ENC_B, ENC_D
    g = torch.Generator().manual_seed(700 + 13 * N + ENC_FAMILIES.index(family))
    qkv = torch.randn(B * N, 3 * D, generator=g)
    if family == "peaked":
        qkv[:, :2 * D] *= ENC_PEAK
        u = ENC_PEAK * torch.randn(B, D, generator=g)
        q, k = qkv[:, :D].view(B, N, D), qkv[:, D:2 * D].view(B, N, D)
        q[:, 0::2] += u[:, None, :]
        k[:, N - 1] = u
    kb = None
    if bias_kind == "float-padding":
        kb = (torch.rand(B, N, generator=g) < 0.3).float()
    elif bias_kind == "inf-prefix":
        kb = torch.zeros(B, N)
        for b, n in enumerate((N, max(1, (N + 1) // 2 - 3), 1)):
            kb[b, n:] = float("-inf")
    elif bias_kind == "inf-first-tile":
        kb = torch.zeros(B, N)
        kb[:, :TILE if N > TILE else max(N - 1, 0)] = float("-inf")
    if kb is not None:
        assert bool((kb > float("-inf")).any(dim=1).all())
    return dict(name=f"enc-{family}-N{N}-{bias_kind}", family=family, B=B, N=N, qkv=qkv.contiguous(), key_bias=kb)


def encoder_error(got, ref64):
    return float((got.to(ref64.device).double() - ref64).abs().max() / max(1.0, float(ref64.abs().max())))


@functools.lru_cache(maxsize=None)
def encoder_ref(family, N, bias_kind, dtype):
    c = encoder_case(family, N, bias_kind)
    return RA.encoder_attention(c["qkv"], c["key_bias"], c["B"], c["N"], ENC_HEADS, dtype)


@functools.lru_cache(maxsize=None)
def encoder_pooled_chain_distance(family):
    return max(encoder_error(encoder_ref(family, N, kb, torch.float32)[0], encoder_ref(family, N, kb, torch.float64)[0])
               for N in ENC_LENGTHS for kb in ENC_BIAS)


def encoder_bound(family):
    rule = 3.0 * encoder_pooled_chain_distance(family)
    return min(rule, CAP) if family == "flat" else rule
